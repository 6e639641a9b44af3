"""The arithmetic of a mix (csrc/gsc_mix.h, exported as ``gsc_mix_model``)
against the definition of include/soundchunks.h in numpy int64, without a GPU:
``y = clamp((sum_k gain_k * x_k + 16384) >> 15, -32768, 32767)``.  The kernels of
``gsc_crop_binding_mix`` accumulate and round with the same functions
(tests/test_gpu_mix.py holds them on the device).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import soundchunks_amd

    return soundchunks_amd.load()


def model(x, gain):
    """The definition for rows of terms: x, gain int64 [N, n] -> int64 [N]."""
    s = (np.asarray(gain, np.int64) * np.asarray(x, np.int64)).sum(axis=1)
    return np.clip((s + 16384) >> 15, -32768, 32767)


def mix(lib, x, gain):
    """gsc_mix_model row by row: x, gain [N, n] -> int64 [N]."""
    x = np.ascontiguousarray(x, np.int16)
    gain = np.ascontiguousarray(gain, np.int64)
    assert x.shape == gain.shape
    out = np.empty(len(x), np.int64)
    y = ctypes.c_int16(0)
    i16p, llp = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_longlong)
    for i in range(len(x)):
        assert lib.gsc_mix_model(x[i].ctypes.data_as(i16p), gain[i].ctypes.data_as(llp), x.shape[1],
                                 ctypes.byref(y)) == 0
        out[i] = y.value
    return out


ALL = np.arange(-32768, 32768, dtype=np.int64)[:, None]


def test_unity_is_identity(lib):
    assert np.array_equal(mix(lib, ALL, np.full_like(ALL, 32768)), ALL[:, 0])


def test_inversion(lib):
    got = mix(lib, ALL, np.full_like(ALL, -32768))
    want = -ALL[:, 0]
    want[0] = 32767  # -(-32768) clamps
    assert np.array_equal(got, want)
    assert np.array_equal(got, model(ALL, np.full_like(ALL, -32768)))


def test_rounding_at_half(lib):
    assert mix(lib, [[1]], [[16384]]).tolist() == [1]
    assert mix(lib, [[-1]], [[16384]]).tolist() == [0]
    # every odd sample at gain one half: half up, not away from zero
    got = mix(lib, ALL, np.full_like(ALL, 16384))
    assert np.array_equal(got, (ALL[:, 0] + 1) >> 1)


def test_sums_saturate(lib):
    unity = [[32768, 32768]]
    assert mix(lib, [[32767, 32767]], unity).tolist() == [32767]
    assert mix(lib, [[-32768, -32768]], unity).tolist() == [-32768]
    assert mix(lib, [[32767, -32768]], unity).tolist() == [-1]


def test_extremes_stay_in_64_bits(lib):
    big = 1 << 20
    for rail, g, want in ((32767, big, 32767), (-32768, big, -32768), (32767, -big, -32768), (-32768, -big, 32767)):
        x, gain = np.full((1, 256), rail), np.full((1, 256), g)
        assert abs(int(rail) * g * 256) < 1 << 63
        assert mix(lib, x, gain).tolist() == [want] == model(x, gain).tolist()
    # the largest partial sums cancelling to something small
    x, gain = np.full((1, 256), 32767), np.full((1, 256), big)
    gain[0, 1::2] = -big
    gain[0, -1] = -big + 3
    assert mix(lib, x, gain).tolist() == model(x, gain).tolist() == [3]


def test_random_terms(lib):
    rng = np.random.default_rng(11)
    for n, span, cases in ((1, 1 << 20, 2000), (2, 1 << 16, 3000), (3, 40000, 3000), (5, 1 << 20, 1500),
                           (256, 1 << 20, 500)):
        x = rng.integers(-32768, 32768, (cases, n))
        gain = rng.integers(-span, span + 1, (cases, n))
        assert np.array_equal(mix(lib, x, gain), model(x, gain)), (n, span)


def test_refusals(lib):
    i16p, llp = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_longlong)
    x, y = (ctypes.c_int16 * 2)(5, 6), ctypes.c_int16(0x5555)
    good = (ctypes.c_longlong * 2)(32768, 32768)
    for gains in ((32768, (1 << 20) + 1), (-(1 << 20) - 1, 0)):
        assert lib.gsc_mix_model(x, (ctypes.c_longlong * 2)(*gains), 2, ctypes.byref(y)) == -1
    for n in (0, -1, 257):
        assert lib.gsc_mix_model(x, good, n, ctypes.byref(y)) == -1
    assert lib.gsc_mix_model(i16p(), good, 2, ctypes.byref(y)) == -1
    assert lib.gsc_mix_model(x, llp(), 2, ctypes.byref(y)) == -1
    assert lib.gsc_mix_model(x, good, 2, i16p()) == -1
    assert y.value == 0x5555  # none of them wrote


def test_symbols_present(lib):
    import soundchunks_amd as sc

    assert hasattr(lib, "gsc_crop_binding_mix") and hasattr(lib, "gsc_mix_model")
    assert callable(sc.CropBinding.mix) and callable(sc.CropBinding.mix_tile)
