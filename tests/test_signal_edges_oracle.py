"""The edge-signal matrix (edge_signals.py) does reach the encoder's corner
cases -- checked on the oracle alone, so that an edit of the signals cannot
quietly empty test_gpu_signal_edges.py.  These are floors on what the matrix
must contain, not measurements of it.
"""
from __future__ import annotations

import numpy as np
import pytest

import edge_signals as es


@pytest.fixture(scope="module")
def survey(oracle):
    """One pass over the matrix: chunk counts of every frame, traces of the checked frames."""
    traces = es.Traces(oracle)
    counts = {e: es.frame_chunk_counts(oracle, e) for e in es.MATRIX}
    checked = {e: traces.checked(e) for e in es.MATRIX}
    return counts, checked


def test_matrix_shape():
    m = es.MATRIX
    assert len(set(m)) == len(m)
    for s in es.SIGNALS:
        mine = [e for e in m if e.signal == s]
        assert {e.cs for e in mine} == set(es.CHUNK_SIZES)
        assert {e.ch for e in mine} == {1, 2} and {e.bd for e in mine} == {8, 12}
        for cs in es.FULL_CS:
            assert {(e.ch, e.bd) for e in mine if e.cs == cs} == {(1, 8), (1, 12), (2, 8), (2, 12)}
        # the single-combination ChunkSizes alternate through all four as well
        assert len({(e.ch, e.bd) for e in mine if e.cs not in es.FULL_CS}) == 4
    assert set(es.STAGE_CS) <= set(es.FULL_CS) and set(es.REPEATED) <= set(es.SIGNALS)


def test_signals_as_specified():
    t = np.arange(es.N_SAMPLES)
    for s in es.SIGNALS:
        p = es.pcm(s, 2)
        assert p.dtype == np.int16 and p.shape == (es.N_SAMPLES, 2)
        x = p[:, 0].astype(np.int64)
        np.testing.assert_array_equal(p[:, 1], np.clip(-x[::-1], -32767, 32767))
        np.testing.assert_array_equal(es.pcm(s, 1)[:, 0], x)
        assert len(es.wav(s, 2)) == 44 + 4 * es.N_SAMPLES and len(es.wav(s, 1)) == 44 + 2 * es.N_SAMPLES
    sig = {s: es.pcm(s, 1)[:, 0].astype(np.int64) for s in es.SIGNALS}
    assert not sig["silence"].any()
    assert set(sig["square_fs"].tolist()) == {32767, -32768} and sig["square_fs"][36] == 32767 \
        and sig["square_fs"][37] == -32768
    assert 0.25 < (sig["min16_mix"] == -32768).mean() < 0.35
    assert (sig["dc"] == 12345).all()
    assert sig["impulse"][t % 97 != 0].max() == 0 and sig["impulse"][[0, 97, 194]].tolist() == [1, -1, 1]
    assert (sig["nyquist"][0::2] == 20000).all() and (sig["nyquist"][1::2] == -20000).all()
    assert set(sig["lsb"].tolist()) == {-1, 0, 1}
    assert sig["ramp"][0] == -32768 and sig["ramp"][-1] == 32767 and (np.diff(sig["ramp"]) >= 0).all()
    assert sig["uniform"].min() < -32000 and sig["uniform"].max() > 32000


def test_attenuation_dividers_reached(survey):
    _, checked = survey
    att = {tr["atten_div"] for frames in checked.values() for _, tr in frames}
    assert 1 in att and 64 in att  # the first law and the last lane
    assert len(att) >= 20, sorted(att)
    assert min(att) >= 1 and max(att) <= 64


def test_frame_sizes_reached(survey):
    counts, checked = survey
    n = np.concatenate(list(counts.values()))
    assert int((n == 0).sum()) >= 1
    assert int((n == 1).sum()) >= 100
    assert int((n > es.K).sum()) >= 50
    for e, frames in checked.items():  # the cut computed here is the oracle's own
        for f, tr in frames:
            assert tr["N"] == counts[e][f] and tr["K"] == es.K and tr["D"] == 2 * e.cs
    # the checked subset of a long entry holds its empty frame and one-chunk frames
    for e in es.entries(("square_fs",), (1,)):
        assert len(counts[e]) > es.MAX_FRAMES
        got = [tr["N"] for _, tr in checked[e]]
        assert 16 <= len(got) <= 17 and 0 in got and e.ch in got


def test_identical_points_reached(survey):
    _, checked = survey
    same = zero = 0
    for frames in checked.values():
        for _, tr in frames:
            d = tr["dataset"]
            if tr["N"] > tr["K"] and (d.view(np.uint32) == d.view(np.uint32)[0]).all():
                if d.any():
                    same += 1
                else:
                    zero += 1
    assert same >= 1  # N > K rows, all the same non-zero vector
    assert zero >= 1  # N > K all-zero rows


def test_stage_frames_exist(oracle):
    """The stage checks have frames to run on, entry by entry: every entry of
    es.STAGE has N > K frames (three; the square's one frame at ChunkSize 13),
    and no candidate left out of es.STAGE has any.  Every repeated-point
    signal but the square is there at every stage ChunkSize, ChunkSize 16
    (D = 32) and mono at ChunkSize 8 through the 6600-sample variants."""
    for e in es.STAGE_CANDIDATES:
        n = es.frame_chunk_counts(oracle, e)
        big = int((n > es.K).sum())
        if e not in es.STAGE:
            assert big == 0, (e.id, n.tolist()[:8])
        else:
            assert big >= (1 if e.signal == "square_fs" else 3), (e.id, n.tolist()[:8])
            assert len(n) <= es.MAX_FRAMES  # so the stage tests look at every one of them
    for s in es.REPEATED:
        if s != "square_fs":
            assert {e.cs for e in es.STAGE if e.signal == s} == set(es.STAGE_CS), s
            assert {(e.cs, e.ch) for e in es.STAGE if e.signal == s} >= {(1, 1), (4, 1), (8, 1), (16, 2), (13, 2)}, s
    assert {(e.cs, e.ch) for e in es.STAGE if e.signal == "square_fs"} == {(13, 1), (13, 2)}


@pytest.mark.parametrize("signal", ["square_fs", "min16_mix"])
def test_min16_sample_inside_a_chunk(oracle, signal):
    for e in es.entries((signal,)):
        x = es.pcm(signal, e.ch)
        st, en = oracle.frame_bounds(e.wav, e.argv)
        inside = np.zeros(es.N_SAMPLES, dtype=bool)
        for a, b in zip(st, en):
            inside[a:min(b, es.N_SAMPLES - 1) + 1] = True
        assert ((x == -32768).any(axis=1) & inside).any(), e.id


def _sign_sums(s):
    """ComputeDstAttributes' two sums over one chunk's f64 samples, in its order."""
    p1 = p2 = 0.0
    for v in s:
        if v < 0:
            p1 -= v
    for v in s:
        if v > 0:
            p2 += v
    return p1, p2


def test_nyquist_sign_and_reverse_ties(oracle):
    found = 0
    for e in es.entries(("nyquist",), tuple(cs for cs in es.CHUNK_SIZES if cs % 2 == 0)):
        samp = es.pcm("nyquist", e.ch).astype(np.float64) / 32767.0  # TEncoder.Load
        st, en = oracle.frame_bounds(e.wav, e.argv)
        for j in range(e.ch):
            s = samp[st[0]:st[0] + e.cs, j]  # the first chunk of the first frame
            assert en[0] - st[0] + 1 >= e.cs
            p1, p2 = _sign_sums(s.tolist())
            assert p1 == p2 and p1 > 0, e.id  # the `neg` tie
            h1 = h2 = 0.0
            for v in s[:e.cs // 2].tolist():
                h1 += abs(v)
            for v in s[e.cs // 2:].tolist():
                h2 += abs(v)
            assert h1 == h2, e.id  # and the `rev` tie
            found += 1
    assert found >= 8
