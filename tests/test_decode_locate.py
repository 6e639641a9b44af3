"""``gsc_index_locate`` (the host lookup under the crop decode) without a GPU:
frame, symbol row, position inside the chunk and checkpoint of a per-channel
sample position, against ``np.searchsorted`` over the arrays ``Index`` exposes.
"""
from __future__ import annotations

import numpy as np
import pytest

import gsc_writer as gw
from golden.cases import HERE

GOLDENS = sorted(p.stem for p in HERE.glob("*.gsc"))


def _crafted():
    rng = np.random.default_rng(31)
    a = gw.random_frame(rng, 600, ch=2, count=300, cs=5, bd=12)
    b = gw.random_frame(rng, 399, ch=3, count=40, cs=3)
    e2, e3 = gw.random_frame(rng, 0, ch=2, count=3, cs=4), gw.random_frame(rng, 0, ch=3, count=0, cs=7)
    return {
        "empty_frame_0": e2 + a + gw.random_frame(rng, 14, ch=2, count=9, cs=1),
        "empty_middle_frame": a + e2 + e2 + gw.random_frame(rng, 260, ch=2, count=9, cs=16),
        "empty_last_frame": a + e2,
        "three_channels": e3 + b + e3 + gw.random_frame(rng, 3 * 130, ch=3, count=1000, cs=1),
        "one_sample": gw.random_frame(rng, 1, ch=1, count=2, cs=1),
    }


CRAFTED = _crafted()


def _check(ix):
    import soundchunks_amd as sc

    S = sc.Decoder.checkpoint_symbols()
    first, n = ix.first_sample, ix.samples_per_channel
    assert n > 0
    rng = np.random.default_rng(n)
    pos = {0, n - 1, *rng.integers(0, n, 64).tolist()}
    for edge in first:
        pos.update(int(edge) + d for d in (-1, 0, 1))
    cp_first = np.concatenate([[0], np.cumsum(-(-ix.frame_length * ix.channels // S))])  # ceil(nsym / S) per frame
    for s in sorted(p for p in pos if 0 <= p < n):
        fr, row, within, cp = ix.locate(s)
        want = int(np.searchsorted(first, s, side="right")) - 1
        assert fr == want and ix.frame_length[fr] > 0, s
        local = s - int(first[fr])
        cs = int(ix.chunk_size[fr])
        assert (row, within) == (local // cs, local % cs), s
        assert cp == int(cp_first[fr]) + row * ix.channels // S, s
        assert cp < cp_first[fr + 1], s
    return len(pos)


@pytest.mark.parametrize("name", GOLDENS)
def test_locate_on_goldens(name):
    import soundchunks_amd as sc

    _check(sc.Decoder.index((HERE / f"{name}.gsc").read_bytes()))


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_locate_on_crafted_streams(name):
    import soundchunks_amd as sc

    ix = sc.Decoder.index(CRAFTED[name])
    _check(ix)
    if name == "empty_frame_0":
        assert ix.locate(0)[0] == 1
    if name == "empty_middle_frame":
        assert ix.locate(1500 - 1)[0] == 0 and ix.locate(1500)[:3] == (3, 0, 0)
    if name == "empty_last_frame":
        assert ix.locate(ix.samples_per_channel - 1)[0] == 0


@pytest.mark.parametrize("name", ["tiny_passthrough_cs8", "syn8s_c2_cs8_cpf4096"])
def test_out_of_range_is_refused_with_a_message(name):
    import ctypes

    import soundchunks_amd as sc

    ix = sc.Decoder.index((HERE / f"{name}.gsc").read_bytes())
    for s in (-1, ix.samples_per_channel, ix.samples_per_channel + 1, -2 ** 62, 2 ** 62):
        with pytest.raises(sc.GscError) as e:
            ix.locate(s)
        assert str(s) in str(e.value)
    # the C entry point itself, with every output pointer NULL
    lib = sc.load()
    assert lib.gsc_index_locate(ix._h, -1, None, None, None, None) < 0 and lib.gsc_last_error()
    assert lib.gsc_index_locate(ix._h, 0, None, None, None, None) == 0
    assert lib.gsc_index_locate(None, 0, None, None, None, None) < 0
    fr = ctypes.c_int(-1)
    assert lib.gsc_index_locate(ix._h, ix.samples_per_channel - 1, ctypes.byref(fr), None, None, None) == 0
    assert fr.value == ix.frame_count - 1


def test_timing_struct_keeps_its_offsets():
    """h2d_bytes is appended: the fields before it stay where they were."""
    from soundchunks_amd._lib import GscDecodeTiming

    assert [f for f, _ in GscDecodeTiming._fields_][-1] == "h2d_bytes"
    assert GscDecodeTiming.samples.offset == 64 and GscDecodeTiming.h2d_bytes.offset == 72
