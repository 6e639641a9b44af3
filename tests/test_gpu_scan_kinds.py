"""The batched scan's two instantiations per shape (gsc_scan.hip): PLAIN for
frames with K = 2^LOGK finite centroids and the slab's own colCount, the
general one for NaN rows, K below the layout's power of two and padded slabs.
The kind is decided on the device before every batched launch
(scan_classify_kernel) and recorded per frame (ReduceFrame::plain,
plain_passes), which GSC_SCAN_DEBUG / GSC_FRAME_STATS print.

Every scan here runs in a fresh child process (the environment switches are
read there) and is compared with the oracle's KNNScanReduce: clusters,
centroids bit for bit, pass count.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

import numpy as np
import pytest

from scan_frames import ROOT, bits as _bits, run_child

pytestmark = pytest.mark.gpu
PASSES = 3
N, K_POW2, K_ODD = 3000, 512, 485

# plain + NaN rows + K = 485 in one launch (both kernels work on one frame
# array, side by side); then each kernel's empty-grid case
LAUNCHES = {"mixed": ["plain", "nan", "odd"], "plain_only": ["plain", "plain2"], "general_only": ["nan", "odd"]}


def _inputs(d):
    rng = np.random.default_rng(100 + d)
    frames = {}
    for name in ("plain", "plain2", "nan", "odd"):
        x = rng.standard_normal((N, d)).astype(np.float32)
        x[:, d // 2:] *= 1e-5  # the cepstrum half's scale (encoder.lpr:1700-1716)
        c = x[rng.choice(N, K_POW2, replace=False)].copy()
        if name == "nan":
            c[[5, 100, 511]] = np.nan  # rows that stay NaN for the whole frame
        if name == "odd":
            c = c[:K_ODD].copy()
        frames[name] = (x, c)
    return frames


def _run_child(tmp_path, d, extra_env):
    """Launches of several frames through the library's internal multi-frame
    scan entry (scan_frames.py: caller centroids, a K per frame, one launch),
    then one single-frame scan through the C ABI with a NaN row."""
    frames = _inputs(d)
    launches = [(launch, "frames", names) for launch, names in LAUNCHES.items()] + [("abi", "abi", ["nan"])]
    env = dict(GSC_SCAN_MAX_PASSES=str(PASSES), GSC_SCAN_DEBUG="1", **extra_env)
    got, err = run_child(tmp_path, frames, launches, env)
    return frames, got, err


_ORACLE = {}


def _oracle_scan(oracle, d, name, frames):
    """The oracle's KNNScanReduce of one frame, computed once per (d, frame)."""
    if (d, name) not in _ORACLE:
        _ORACLE[d, name] = oracle.scan_reduce(frames[name][0], frames[name][1], 3, PASSES)
    return _ORACLE[d, name]


def _check_frame(oracle, d, frames, got, launch, name):
    oc, ocl, on = _oracle_scan(oracle, d, name, frames)
    key = f"{launch}/{name}"
    assert int(got[key + "/meta"][0]) == on == PASSES, key
    np.testing.assert_array_equal(got[key + "/cl"], ocl, err_msg=key)
    nan = np.isnan(oc)
    np.testing.assert_array_equal(np.isnan(got[key + "/c"]), nan, err_msg=key)
    np.testing.assert_array_equal(_bits(np.where(nan, 0, got[key + "/c"])), _bits(np.where(nan, 0, oc)), err_msg=key)


@pytest.mark.parametrize("d", [8, 16])
def test_each_kind_runs_in_its_instantiation(oracle, tmp_path, d):
    """One launch of a plain frame, a frame with NaN centroid rows and a frame
    with K = 485: each runs in the instantiation it belongs to and all three
    are bit-exact against the oracle; then a plain-only and a general-only
    launch, and the NaN frame alone through the C ABI (classified on that path
    too).  The oracle's scan returns no residual, so the residual is compared
    between the launches instead: a frame's value must not depend on its
    neighbours or on which kernels the launch had work for."""
    frames, got, err = _run_child(tmp_path, d, {})
    for launch, names in LAUNCHES.items():
        for name in names:
            _check_frame(oracle, d, frames, got, launch, name)
            it, pl, pp = (int(v) for v in got[f"{launch}/{name}/meta"])
            want_plain = name.startswith("plain")
            assert (pl, pp) == ((1, it) if want_plain else (0, 0)), (launch, name, pl, pp, it)
    for name in ("plain", "nan", "odd"):
        other = "plain_only" if name == "plain" else "general_only"
        a, b = float(got[f"mixed/{name}/err"]), float(got[f"{other}/{name}/err"])
        assert a == b or (np.isnan(a) and np.isnan(b)), (name, a, b)
    _check_frame(oracle, d, frames, got, "abi", "nan")
    assert re.findall(r"kind (\w+) plain_passes (\d+)", err) == [("general", "0")], err[-1500:]


def test_product_build_ignores_scan_kb(oracle, tmp_path):
    """GSC_SCAN_KB is an experiment switch: not compiled into the product
    kernels (tests/test_scan_kinds_resources.py: they take no `opts`), said once
    on stderr however many scans run, and the results are what they are without it."""
    frames, got, err = _run_child(tmp_path, 16, {"GSC_SCAN_KB": "16"})
    assert err.count("GSC_SCAN_KB set, but the scan experiments are not compiled into this build") == 1, err[-1500:]
    for name in LAUNCHES["mixed"]:
        _check_frame(oracle, 16, frames, got, "mixed", name)


def _encode_frame_kinds(wav_path, argv):
    code = (f"import sys; sys.path[:0]=[{str(ROOT)!r},{str(ROOT / 'tests')!r}];"
            f"import soundchunks_amd as sc; sc.Encoder({argv!r}).encode(open({str(wav_path)!r},'rb').read())")
    env = dict(os.environ, GSC_SCAN_MAX_PASSES="1", GSC_FRAME_STATS="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-2000:]
    return {int(f): (k, int(p), int(it)) for f, it, k, p in
            re.findall(r"frame (\d+): N \d+ passes (\d+) .* kind (\w+) plain_passes (\d+)", r.stderr)}, r.stderr


def test_encode_routes_frames_by_device_classification(oracle, tmp_path):
    """Frames that are plain by K and colCount, entered through `encode`.  Frame
    1 of the corpus' 60.wav at -cs8 -cpf4096 has over a thousand NaN rows in its
    yakmo means (seeds that won no point; test_gpu_scan.py asserts that on the
    oracle's trace); a short synthetic clip has none (the oracle's trace, here).
    Only the classification on the device can tell the two apart: the first runs
    in the general kernel, the second runs every pass in the PLAIN one."""
    from soundchunks_amd.synth import synth_wav

    kinds, err = _encode_frame_kinds(ROOT / "tests" / "golden" / "lame_test" / "60.wav", ["-cs8", "-cpf4096"])
    assert 1 in kinds, err[-1500:]
    assert kinds[1][:2] == ("general", 0), kinds
    for k, p, it in kinds.values():  # every frame of the launch: all of its passes in its own kernel
        assert p == (it if k == "plain" else 0), kinds
    clip, argv = tmp_path / "clip.wav", ["-cs8", "-cpf256"]
    clip.write_bytes(synth_wav(0.6))  # one frame, 6615 chunks, K = 256
    assert not np.isnan(oracle.trace_frame(clip.read_bytes(), argv, 0)["yakmo"]).any()
    kinds, err = _encode_frame_kinds(clip, argv)
    assert 0 in kinds, err[-1500:]
    k, p, it = kinds[0]
    assert (k, p) == ("plain", it) and it == 1, kinds
