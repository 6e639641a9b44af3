"""The crop planner the bound kernels run (csrc/gsc_crop_plan.h, exported for
the host as ``gsc_crop_plan_model`` / ``Index.plan_crop``) against the
definitions: the frames of a crop's source range are ``Index.locate``'s, of a
run of frames that start at the same sample the last one; the written count is
``min(count, ceil((samples - begin) L / M))``; the source range is the filter's
reach clipped to the stream.  Host only: the index is the host walk's.
"""
from __future__ import annotations

from math import gcd

import numpy as np
import pytest

import gsc_writer as gw
from golden.cases import HERE

GOLDENS = ["square_empty_frame0_cs4", "syn2s_cs7_mono_cbd12", "hihat_cs8_cpf256"]


def many_frames(seed=7, ch=1, rate=32000, cs=3):
    """About 30 short frames (3 to 40 symbol rows of ChunkSize 3) with runs of
    empty frames at the start (3), in the middle (2 and 4) and at the end (3)."""
    rng = np.random.default_rng(seed)

    def full(rows, policy="minimal"):
        return gw.random_frame(rng, ch * rows, ch=ch, count=40, cs=cs, rate=rate, policy=policy)

    def empty():
        return gw.random_frame(rng, 0, ch=ch, count=5, cs=cs, rate=rate)

    rows = [int(r) for r in rng.integers(3, 41, 21)]
    parts = [empty(), empty(), empty()]
    for i, r in enumerate(rows):
        parts.append(full(r, "always" if i % 3 == 0 else "minimal"))
        if i == 6:
            parts += [empty(), empty()]
        if i == 13:
            parts += [empty(), empty(), empty(), empty()]
    parts += [empty(), empty(), empty()]
    return b"".join(parts)


@pytest.fixture(scope="module")
def sc():
    import soundchunks_amd

    return soundchunks_amd


def shape_of(sc, fi, fo):
    """(L, M, T) of a pair of rates; (1, 1, 0) when nothing is resampled."""
    if fo is None or fo == fi:
        return 1, 1, 0
    g = gcd(fi, fo)
    return fo // g, fi // g, sc.Decoder.resample_table(fi, fo).shape[1] // 2


def crops_of(ix, length, seed):
    n = ix.samples_per_channel
    rng = np.random.default_rng(seed)
    crops = [(0, 0), (0, 1), (0, length), (n, 0), (n, length), (max(n - 1, 0), 1), (max(n - 1, 0), length)]
    first = [int(v) for v in ix.first_sample]
    for i in range(ix.frame_count):
        a, b = first[i], first[i + 1]  # the frame holds [a, b)
        for s in {a, max(b - 1, a)}:
            if s < n:
                crops += [(s, 1), (s, 2), (s, length)]          # starting at the frame's first / last sample
                for c in (1, 2, 7):                              # ... and ending there
                    if s - c + 1 >= 0:
                        crops.append((s - c + 1, c))
    crops += [(int(b), int(c)) for b, c in zip(rng.integers(0, n + 1, 64), rng.integers(0, length + 1, 64))]
    return crops


def check_stream(sc, gsc, out_rate, length=500, seed=1):
    ix = sc.Decoder.index(gsc)
    n, fi = ix.samples_per_channel, ix.sample_rate
    L, M, T = shape_of(sc, fi, out_rate)
    runs = 0
    for b, c in crops_of(ix, length, seed):
        p = ix.plan_crop(b, c, length, rate=out_rate)
        want = min(c, -((-(n - b) * L) // M))
        assert p["status"] == 0 and p["written"] == want, (b, c, p, want)
        if want == 0:
            assert (p["f0"], p["f1"], p["src_begin"], p["src_end"]) == (0, 0, 0, 0), (b, c, p)
            continue
        last = (b * L + (want - 1) * M) // L
        assert last < n
        assert p["src_begin"] == max(b - max(T - 1, 0), 0) and p["src_end"] == min(last + T + 1, n), (b, c, p)
        fa, fb = ix.locate(p["src_begin"])[0], ix.locate(p["src_end"] - 1)[0]
        assert (p["f0"], p["f1"] - 1) == (fa, fb), (b, c, p, fa, fb)
        # of frames that start at the same sample the span starts (ends) in the last one
        for f in (fa, fb):
            if f > 0 and ix.first_sample[f - 1] == ix.first_sample[f]:
                runs += 1
            assert ix.first_sample[f + 1] > ix.first_sample[f]
    ix.close()
    return runs


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(sc, name):
    gsc = (HERE / f"{name}.gsc").read_bytes()
    for rate in (None, 44100, 16000):
        check_stream(sc, gsc, rate, length=3000, seed=len(name))


@pytest.mark.parametrize("fi,fo", [(32000, None), (32000, 44100), (48000, 16000)])
def test_many_frames(sc, fi, fo):
    gsc = many_frames(rate=fi)
    ix = sc.Decoder.index(gsc)
    first = [int(v) for v in ix.first_sample]
    assert 28 <= ix.frame_count <= 36
    # runs of empty frames at the start, in the middle and at the end
    assert first[0] == first[3] == 0 and first[-1] == first[-4] == ix.samples_per_channel
    assert sum(1 for i in range(4, ix.frame_count - 4) if first[i] == first[i + 1]) == 6
    ix.close()
    assert check_stream(sc, gsc, fo) > 0  # crops did start or end behind a run of empty frames


def test_bad_crops(sc):
    ix = sc.Decoder.index((HERE / "syn2s_cs7_mono_cbd12.gsc").read_bytes())
    n, length = ix.samples_per_channel, 100
    for rate in (None, 16000):
        bad = [(dict(stream=-1), 1), (dict(stream=2, nstreams=2), 1), (dict(begin=-1), 2), (dict(begin=n + 1, count=0), 2),
               (dict(count=-1), 3), (dict(count=length + 1), 3)]
        for kw, status in bad:
            args = dict(begin=10, count=5, length=length, rate=rate)
            args.update(kw)
            p = ix.plan_crop(**args)
            assert p["status"] == status and p["written"] == -1, (kw, p)
            assert (p["f0"], p["f1"], p["src_begin"], p["src_end"]) == (0, 0, 0, 0), (kw, p)
        # their good neighbours
        for kw in (dict(stream=1, nstreams=2), dict(begin=0), dict(begin=n, count=0), dict(begin=n), dict(count=0),
                   dict(count=length)):
            args = dict(begin=10, count=5, length=length, rate=rate)
            args.update(kw)
            assert ix.plan_crop(**args)["status"] == 0, kw
    with pytest.raises(sc.GscError, match="44100.*1000"):  # a pair of rates without a resampler is an error
        ix.plan_crop(0, 5, length, rate=1000)
    ix.close()
