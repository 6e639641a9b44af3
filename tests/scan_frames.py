"""Stage-level access to the batched scan for the GPU tests (a helper module,
imported by test_gpu_scan_kinds.py and test_gpu_scan_matrix.py).

  * the ctypes signature of the library's internal multi-frame entry
    gsc_scan_reduce_frames (caller centroids, a K per frame, any colCount
    1..32, one launch; out per frame: passes, kind, PLAIN passes, residual);
  * run_child: every launch of a test in ONE fresh child process with a
    timeout (the environment switches are read there, and a fault ends the
    child, not pytest);
  * oracle_scan: the oracle's KNNScanReduce, cached per process by the input;
  * assert_matches_oracle: the comparison used everywhere -- pass count,
    clusters, NaN positions, every other centroid word bit for bit.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
PRECISION = 3

# restype and argtypes of gsc_scan_reduce_frames(nf, d0, ns, x, ks, centroids,
# clusters, precision, iters, plain, plain_passes, err), as ctypes expressions
# for the child (FP / IP / DP: pointers to float / int / double)
FRAMES_RESTYPE = "ctypes.c_int"
FRAMES_ARGTYPES = "[ctypes.c_int, ctypes.c_int, IP, FP, IP, FP, IP, ctypes.c_int, IP, IP, IP, DP]"

# A launch is (name, route, [frame names]):
#   route "frames": the named frames (one colCount) in one gsc_scan_reduce_frames call;
#   route "abi":    each named frame on its own through gsc_scan_reduce (the C ABI).
# The child writes, per launch and frame, launch/frame/c, /cl, /meta = (passes,
# plain, plain_passes) (-1, -1 on the ABI route, which returns neither) and /err.
CHILD = """
import ctypes, json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import soundchunks_amd as sc
lib = sc.load()
FP, IP, DP = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_int, ctypes.c_double))
fn = lib.gsc_scan_reduce_frames
fn.restype = {restype}
fn.argtypes = {argtypes}
z = np.load({inp!r})
out = {{}}
for launch, route, names in json.loads({launches!r}):
    if route == "abi":
        for n in names:
            c, cl, it = sc.scan_reduce(z["x_" + n], z["c_" + n], precision={precision})
            out[launch + "/" + n + "/c"], out[launch + "/" + n + "/cl"] = c, cl
            out[launch + "/" + n + "/meta"] = np.array([it, -1, -1])
            out[launch + "/" + n + "/err"] = np.nan
        continue
    xs = [z["x_" + n] for n in names]
    cs = [z["c_" + n] for n in names]
    ns = np.array([len(a) for a in xs], dtype=np.int32)
    ks = np.array([len(a) for a in cs], dtype=np.int32)
    x = np.ascontiguousarray(np.concatenate(xs), dtype=np.float32)
    c = np.ascontiguousarray(np.concatenate(cs), dtype=np.float32)
    cl = np.zeros(int(ns.sum()), dtype=np.int32)
    it, pl, pp = (np.zeros(len(names), dtype=np.int32) for _ in range(3))
    err = np.zeros(len(names), dtype=np.float64)
    rc = fn(len(names), x.shape[1], ns.ctypes.data_as(IP), x.ctypes.data_as(FP), ks.ctypes.data_as(IP),
            c.ctypes.data_as(FP), cl.ctypes.data_as(IP), {precision}, it.ctypes.data_as(IP), pl.ctypes.data_as(IP),
            pp.ctypes.data_as(IP), err.ctypes.data_as(DP))
    assert rc == 0, (launch, sc.last_error() if hasattr(sc, "last_error") else rc)
    co = np.cumsum(np.concatenate([[0], ks])); no = np.cumsum(np.concatenate([[0], ns]))
    for i, n in enumerate(names):
        out[launch + "/" + n + "/c"] = c[co[i]:co[i + 1]]
        out[launch + "/" + n + "/cl"] = cl[no[i]:no[i + 1]]
        out[launch + "/" + n + "/meta"] = np.array([it[i], pl[i], pp[i]])
        out[launch + "/" + n + "/err"] = err[i]
np.savez({outp!r}, **out)
"""

# one frame of one launch, as the GPU returned it
FrameResult = namedtuple("FrameResult", "c cl passes plain plain_passes err")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_child(tmp_path, frames, launches, env=None, timeout=150):
    """Run `launches` (see CHILD) over `frames` = {name: (x, c)} in one child
    process.  Returns the child's npz (keys launch/frame/...) and its stderr."""
    inp, outp = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(inp, **{"x_" + k: v[0] for k, v in frames.items()}, **{"c_" + k: v[1] for k, v in frames.items()})
    code = CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), inp=str(inp), outp=str(outp),
                        restype=FRAMES_RESTYPE, argtypes=FRAMES_ARGTYPES, precision=PRECISION,
                        launches=json.dumps([[n, r, list(f)] for n, r, f in launches]))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **(env or {})), capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(outp), r.stderr


def frame_result(got, launch, name):
    key = f"{launch}/{name}"
    it, pl, pp = (int(v) for v in got[key + "/meta"])
    return FrameResult(got[key + "/c"], got[key + "/cl"], it, pl, pp, float(got[key + "/err"]))


_ORACLE = {}


def _key(x, c, max_passes):
    h = hashlib.sha1()
    for a in (x, c):
        a = np.ascontiguousarray(a, dtype=np.float32)
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest(), int(max_passes)


def oracle_scan(oracle, x, c, max_passes=100):
    """The oracle's KNNScanReduce of one frame: (centroids, clusters, passes),
    computed once per process for an input.  Treat the result as read-only."""
    k = _key(x, c, max_passes)
    if k not in _ORACLE:
        _ORACLE[k] = oracle.scan_reduce(x, c, PRECISION, max_passes)
    return _ORACLE[k]


def oracle_scan_many(oracle, frames, max_passes=100):
    """oracle_scan of every frame of {name: (x, c)}, the uncached ones side by
    side (the oracle's scan keeps no state between calls)."""
    todo = {n: f for n, f in frames.items() if _key(f[0], f[1], max_passes) not in _ORACLE}
    if len(todo) > 1:
        oracle.load()
        with ThreadPoolExecutor(max_workers=min(16, len(todo), os.cpu_count() or 1)) as ex:
            list(ex.map(lambda f: oracle_scan(oracle, f[0], f[1], max_passes), todo.values()))
    return {n: oracle_scan(oracle, f[0], f[1], max_passes) for n, f in frames.items()}


def assert_matches_oracle(res, want, what):
    """res: a FrameResult; want: oracle_scan's triple."""
    oc, ocl, on = want
    assert res.passes == on, (what, res.passes, on)
    np.testing.assert_array_equal(res.cl, ocl, err_msg=f"{what}: clusters")
    nan = np.isnan(oc)
    np.testing.assert_array_equal(np.isnan(res.c), nan, err_msg=f"{what}: NaN positions")
    np.testing.assert_array_equal(bits(np.where(nan, 0, res.c)), bits(np.where(nan, 0, oc)),
                                  err_msg=f"{what}: centroid words")
