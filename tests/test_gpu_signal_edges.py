"""HIP encoder vs oracle on full-scale, constant and degenerate signals
(edge_signals.py; run on a real MI355X: pytest -m gpu).

Whole files, the device DSP of every checked frame, and the clustering stages
on the oracle's traces of the frames with N > K.  Every comparison is exact:
bytes for streams, uint32 views for floats (NaN payloads included).  The
oracle runs live; test_signal_edges_oracle.py holds the matrix to the corner
cases it is meant to reach.
"""
from __future__ import annotations

import numpy as np
import pytest

import edge_signals as es

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ids(entries):
    return [e.id for e in entries]


@pytest.fixture(scope="module")
def traces(oracle):
    return es.Traces(oracle)


@pytest.fixture(scope="module")
def oracle_gsc(oracle):
    """The oracle's .gsc of an entry, encoded once per module."""
    done = {}

    def get(e):
        if e not in done:
            done[e] = oracle.encode(e.wav, e.argv)
        return done[e]

    return get


# ---- whole file -----------------------------------------------------------
# the matrix, and the 6600-sample stage variants: at -cs16 only they reach the clustering path
_FILES = es.MATRIX + es.STAGE_EXTRA


@pytest.mark.parametrize("e", _FILES, ids=_ids(_FILES))
def test_file_matches_oracle(oracle_gsc, e):
    import soundchunks_amd as sc

    want = oracle_gsc(e)
    got = sc.Encoder(e.argv).encode(e.wav)
    assert len(got) == len(want)
    assert got == want


_RECON = es.entries(chunk_sizes=es.STAGE_CS)


@pytest.mark.parametrize("e", _RECON, ids=_ids(_RECON))
def test_reconstruction_matches_oracle(oracle, oracle_gsc, e):
    import soundchunks_amd as sc

    ogsc, orec, opsy = oracle.encode_recon(e.wav, e.argv)
    assert ogsc == oracle_gsc(e)
    gsc, rec, psy = sc.Encoder(e.argv).encode_recon(e.wav)
    assert gsc == ogsc
    assert rec.dtype == orec.dtype and rec.shape == orec.shape
    np.testing.assert_array_equal(rec, orec)
    assert np.float64(psy).view(np.uint64) == np.float64(opsy).view(np.uint64)  # bit-identical f64


# ---- DSP, every checked frame ---------------------------------------------
@pytest.mark.parametrize("e", es.MATRIX, ids=_ids(es.MATRIX))
def test_frame_dsp_bit_exact(traces, e):
    import soundchunks_amd as sc

    frames = traces.checked(e)
    assert frames
    assert sc.Encoder(e.argv).frame_count(e.wav) == len(es.frame_chunk_counts(traces.oracle, e))
    for f, tr in frames:
        att, feat = sc.frame_dsp(e.wav, f, e.argv)
        assert att == tr["atten_div"], (f, tr["N"])
        assert feat.shape == tr["dataset"].shape, f
        np.testing.assert_array_equal(_bits(feat), _bits(tr["dataset"]), err_msg=f"frame {f}")


# ---- stages on the traced frames with N > K ---------------------------------
# only the entries that have such frames (edge_signals.STAGE; test_signal_edges_oracle.py checks the list)
_STAGE = es.STAGE


def _big(traces, e):
    big = [(f, tr) for f, tr in traces.checked(e) if tr["N"] > tr["K"]]
    assert big, "no N > K frame: nothing would be compared"
    return big


@pytest.mark.parametrize("e", _STAGE, ids=_ids(_STAGE))
def test_yakmo_seed_means_bit_exact(traces, e):
    import soundchunks_amd as sc

    for f, tr in _big(traces, e):
        c = sc.yakmo_seed_means(tr["dataset"], tr["K"])
        np.testing.assert_array_equal(_bits(c), _bits(tr["yakmo"]), err_msg=f"frame {f}")


@pytest.mark.parametrize("e", _STAGE, ids=_ids(_STAGE))
def test_scan_reduce_bit_exact(traces, e):
    import soundchunks_amd as sc

    for f, tr in _big(traces, e):
        c, cl, passes = sc.scan_reduce(tr["dataset"], tr["yakmo"], precision=3)
        assert passes == tr["scan_iters"], f
        np.testing.assert_array_equal(cl, tr["clusters"], err_msg=f"frame {f}")
        np.testing.assert_array_equal(_bits(c), _bits(tr["scan"]), err_msg=f"frame {f}")


@pytest.mark.parametrize("e", _STAGE, ids=_ids(_STAGE))
def test_knnfit_bit_exact(traces, e):
    import soundchunks_amd as sc

    for f, tr in _big(traces, e):
        best = sc.knnfit_assign(tr["knn_cand"][0::4], tr["knn_query"], tr["knn_eps"])
        np.testing.assert_array_equal(best, tr["knn_best"], err_msg=f"frame {f}")


# ---- many tiny frames in one launch -----------------------------------------
_TINY = [e for e in es.entries(("square_fs",), (1, 4, 16)) if e.ch == 1]


@pytest.mark.parametrize("e", _TINY, ids=_ids(_TINY))
def test_many_tiny_frames_one_launch(oracle, oracle_gsc, e):
    """6001, 1501 and 376 frames of one chunk each (at ChunkSize 1 the first
    has none): every stage's batched launch over all of them at once."""
    import soundchunks_amd as sc

    want = oracle_gsc(e)
    n = es.frame_chunk_counts(oracle, e)
    assert len(n) == es.N_SAMPLES // e.cs + 1
    assert n[0] == (0 if e.cs == 1 else 1) and (n[1:] == 1).all()
    p = sc.Encoder(e.argv).prepare(e.wav)
    try:
        assert p.frame_count == len(n)
        np.testing.assert_array_equal(p.frame_chunks(), n)
        blob, sizes = p.encode_frames()
    finally:
        p.close()
    assert len(sizes) == len(n) and sum(sizes) == len(blob)
    assert blob == want
    got, rate = sc.Decoder().decode(blob)
    pcm, ch, orate = oracle.decode(blob)
    assert rate == orate == es.RATE and ch == 1
    assert got.dtype == np.int16 and got.shape == (len(pcm), 1)
    np.testing.assert_array_equal(got.reshape(-1), pcm)
