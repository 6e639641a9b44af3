"""Every kernel object of the batched scan (gsc_scan.hip gsc_launch_scan_batch)
against the oracle's KNNScanReduce, at small shapes, plus the frames on which
a kernel like this goes wrong and the scan's two other routes.

The dispatch has 15 layouts (feature stride S in 8/16/32 x leaves P = 2^logk in
256..4096; the largest K of a launch picks P) and two instantiations per
layout, PLAIN and general, except the split layout (32, 4096), which has only
the general one: 29 objects.  A frame runs PLAIN when its K is P, its colCount
is S and no centroid row is NaN; the device decides (scan_classify_kernel) and
reports it per frame, and the kind assertions below prove the routing.

What ran each object before this module (stage tests by shape; whole-file
goldens of tests/golden/cases.py by their -cs / -cpf: colCount = 2 cs, a frame
can be plain only when 2 cs is 8, 16 or 32 and K a power of two), and what
runs it here -- `matrix` is test_layout[S-P]: launch A's `plain` /
`plain_short` frames for PLAIN, its `nan_rows` / `below` / `half` frames and
the whole of launch B (colCount S - 2) for general.  The `nan` frame has a row
that is NaN in one coordinate only: the batched kernel hands every pass of such
a frame to the per-search generic kernel (it treated the row as a whole NaN row
and never moved its finite coordinates: every layout failed this frame before
that hand-over), so `nan` checks the hand-over and `nan_rows` the batched
kernel's own NaN paths:

  S   P     PLAIN before                    general before                here
  8   256   golden cs4 cpf256 (fl13000)     golden cs1 cpf256             matrix, edges, routes
  8   512   scan_kinds, parity, goldens     scan_kinds, golden cs2        matrix (+ colCount 2)
  8   1024  grid ties (test_gpu_scan)       golden cs3 cpf1000            matrix
  8   2048  --                              --                            matrix
  8   4096  grid ties, golden cs4 cpf4096   only if a golden has NaN rows matrix
  16  256   parity, goldens cs8 cpf256      only if a golden has NaN rows matrix, routes
  16  512   scan_kinds                      scan_kinds, golden cs5        matrix (+ colCount 10), edges
  16  1024  golden cs8 cpf1024              goldens cpf1000, cs6, cs7     matrix
  16  2048  --                              golden -br128 (K = 1852)      matrix
  16  4096  test_gpu_scan (C2 trace)        test_scan_nan_centroids_k4096 matrix
  32  256   test_scan_d32_one_cu[256]       --                            matrix, routes
  32  512   --                              golden cs9 (colCount 18)      matrix (+ colCount 18)
  32  1024  --                              golden cs15 (colCount 30)     matrix, grid edge
  32  2048  test_scan_d32_one_cu[2048]      golden cs12 cpf2048           matrix
  32  4096  (no such object)                test_gpu_scan (C3 trace)      matrix

Passes: to convergence where P <= 1024; three passes (GSC_SCAN_MAX_PASSES=3,
oracle max_passes 3) where P >= 2048, where the sequential oracle needs
seconds per frame to converge.  Every launch of a test runs in one child
process (scan_frames.py).
"""
from __future__ import annotations

import re

import numpy as np
import pytest

from scan_frames import assert_matches_oracle, frame_result, oracle_scan_many, run_child

pytestmark = pytest.mark.gpu

LAYOUTS = [(s, p) for s in (8, 16, 32) for p in (256, 512, 1024, 2048, 4096)]
SMALLEST_COLS = {8: 2, 16: 10, 32: 18}  # smallest colCount of a stride (its launch: P = 512 only)
CAP = 3

# Generated frames that do not converge below 100 passes in the oracle get
# another seed (P <= 1024 only; above it the passes are capped):
# (colCount, K) -> seed
RESEED = {(32, 129): 4320129, (32, 2): 13320002}

# A frame with all-NaN centroid rows never converges: a query whose descent
# reaches such a row first is answered with it (distance NaN), the residual is
# NaN from then on and `diff <= tol` is false in every pass, for any seed.  So
# the `nan` frames of the uncapped layouts run all 100 passes (kMaxScanIters)
# in the general instantiation, on both sides.


def gen(d0, k, n=None, seed=None):
    rng = np.random.default_rng(d0 * 10000 + k if seed is None else seed)
    n = max(600, 2 * k) if n is None else n
    x = rng.standard_normal((n, d0)).astype(np.float32)
    x[:, d0 // 2:] *= 1e-5  # the cepstrum half's scale (encoder.lpr:1700-1716)
    c = x[rng.choice(n, min(k, n), replace=False)].copy()
    return x, c


def _gen(d0, k):
    return gen(d0, k, seed=RESEED.get((d0, k)))


def with_nans(x, c, partial=True):
    """Rows 0 and K - 1 all NaN, row K / 2 + 1 NaN in its last column only.
    The partly-NaN row sends every pass to the per-search generic kernel, and
    uncapped that is 100 passes: 600 points there (measured: test_layout[32-1024]
    took 12 s with all 2048 points in both NaN frames)."""
    c, k = c.copy(), len(c)
    c[[0, k - 1]] = np.nan
    if partial:
        c[k // 2 + 1, -1] = np.nan
    return (x[:600] if k <= 1024 else x), c


def launch_a(s, p):
    x, c = _gen(s, p)
    return {
        "plain": (x, c),
        # 600 rows of another seed over the same centroids: another pass count, so another round
        "plain_short": (gen(s, p, n=600, seed=7 + s * 10000 + p)[0], c),
        "nan": with_nans(x, c),
        # whole NaN rows only (what yakmo's 0/0 means are): these stay in the batched general kernel
        "nan_rows": with_nans(x, c, partial=False),
        "below": _gen(s, p - 1),
        "half": _gen(s, p // 2 + 1),
    }


def launch_b(d0, p):
    x, c = _gen(d0, p)
    return {"k": (x, c), "k_nan": with_nans(x, c), "k_below": _gen(d0, p - 1)}


def _is_nan_like_input(oc, c_in):
    return np.array_equal(np.isnan(oc), np.isnan(c_in))


@pytest.mark.parametrize("s,p", LAYOUTS, ids=[f"{s}-{p}" for s, p in LAYOUTS])
def test_layout(oracle, tmp_path, s, p):
    """Launch A (colCount = S: plain, plain_short, nan, nan_rows, below, half), launch B
    (colCount = S - 2, the padded slab: K = P, the same with NaN rows, K = P - 1)
    and, at P = 512, the stride's smallest colCount: every frame against the
    oracle and in the instantiation it belongs to."""
    capped = p >= 2048
    groups = {"A": launch_a(s, p), "B": launch_b(s - 2, p)}
    if p == 512:
        groups["C"] = launch_b(SMALLEST_COLS[s], p)
    frames = {f"{g}_{n}": f for g, fs in groups.items() for n, f in fs.items()}
    launches = [(g, "frames", [f"{g}_{n}" for n in fs]) for g, fs in groups.items()]
    want = oracle_scan_many(oracle, frames, CAP if capped else 100)

    # the cases are what they claim to be, by the oracle alone
    oc, ocl, on = want["A_plain"]
    assert len(np.unique(ocl)) == p, "the plain frame leaves clusters unused"
    for n, (oc, ocl, on) in want.items():
        has_nan_rows = bool(np.isnan(frames[n][1]).all(axis=1).any())
        assert on == (CAP if capped else 100) if capped or has_nan_rows else on < 100, (n, on)
        assert _is_nan_like_input(oc, frames[n][1]), n
    if not capped:
        assert want["A_plain"][2] != want["A_plain_short"][2], "plain and plain_short finish in the same round"

    got, _ = run_child(tmp_path, frames, launches, {"GSC_SCAN_MAX_PASSES": str(CAP)} if capped else {})
    for g, fs in groups.items():
        for n in fs:
            key = f"{g}_{n}"
            res = frame_result(got, g, key)
            print(f"{s}-{p} {key}: passes {res.passes} (oracle {want[key][2]}) kind {res.plain} plain_passes {res.plain_passes}")
            assert_matches_oracle(res, want[key], (s, p, key))
            is_plain = g == "A" and n in ("plain", "plain_short") and (s, p) != (32, 4096)
            assert (res.plain, res.plain_passes) == ((1, res.passes) if is_plain else (0, 0)), (s, p, key)


def _edge_frames():
    f = {}
    x, c = gen(16, 512, n=100)  # N below K: the centroids are 512 rows of a larger draw
    f["n_below_k"] = (x, gen(16, 512)[1])
    f["n1_k2_16"] = (gen(16, 2, n=1, seed=11)[0], gen(16, 2, seed=12)[1])
    f["n1_k2_8"] = (gen(8, 2, n=1, seed=13)[0], gen(8, 2, seed=14)[1])
    f["identical"] = (np.full((1500, 8), 0.25, np.float32), np.full((256, 8), 0.25, np.float32))
    x, c = gen(16, 512, n=2000)
    c[100:200] = c[0]  # duplicate rows: zero-spread cuts in ANN's split rule
    f["duplicates"] = (x, c)
    f["cap100"] = gen(6, 2, n=600, seed=60002)
    return f


EDGES = {  # name -> (the oracle's pass count where the frame fixes it, else None: below 100; plain)
    "n_below_k": (None, 1), "n1_k2_16": (None, 0), "n1_k2_8": (None, 0), "identical": (2, 1), "duplicates": (None, 1),
    "cap100": (100, 0),
}


def test_edge_frames(oracle, tmp_path):
    """(16, 512) and (8, 256): N below K, N = 1 with K = 2, all points and
    centroids identical, 100 duplicate centroid rows, and the 100-pass cap
    (kMaxScanIters) at the smallest shape that reaches it; one launch each."""
    frames = _edge_frames()
    want = oracle_scan_many(oracle, frames)
    for n, (passes, _) in EDGES.items():
        print(f"edge {n}: oracle passes {want[n][2]}")
        assert want[n][2] == passes if passes is not None else want[n][2] < 100, (n, want[n][2])
    assert (want["identical"][1] == 255).all()
    got, _ = run_child(tmp_path, frames, [(n, "frames", [n]) for n in frames])
    for n, (_, plain) in EDGES.items():
        res = frame_result(got, n, n)
        assert_matches_oracle(res, want[n], n)
        assert (res.plain, res.plain_passes) == ((1, res.passes) if plain else (0, 0)), n
    assert frame_result(got, "cap100", "cap100").passes == 100 == want["cap100"][2]


def test_edge_integer_grid_ties(oracle, tmp_path):
    """Integer-grid points at colCount 32, K = 1024: exact distance ties
    everywhere.  It does not converge in the oracle: three passes."""
    rng = np.random.default_rng(321024)
    x = rng.integers(-3, 4, (2048, 32)).astype(np.float32)
    frames = {"grid": (x, x[rng.choice(2048, 1024, replace=False)].copy())}
    want = oracle_scan_many(oracle, frames, CAP)
    assert want["grid"][2] == CAP
    got, _ = run_child(tmp_path, frames, [("grid", "frames", ["grid"])], {"GSC_SCAN_MAX_PASSES": str(CAP)})
    res = frame_result(got, "grid", "grid")
    assert_matches_oracle(res, want["grid"], "grid")
    assert (res.plain, res.plain_passes) == (1, CAP)


def _route_frames(s):
    x, c = _gen(s, 256)
    return {"plain": (x, c), "nan": with_nans(x, c), "k2": _gen(s, 2)}


@pytest.mark.parametrize("generic", [False, True], ids=["abi", "generic"])
@pytest.mark.parametrize("s", [8, 16, 32])
def test_other_routes(oracle, tmp_path, s, generic):
    """gsc_scan_reduce (the single-frame C ABI, classified on that path too)
    and, with GSC_SCAN_GENERIC=1, the per-search generic kernel: a plain frame,
    NaN rows and K = 2 at P = 256."""
    frames = _route_frames(s)
    want = oracle_scan_many(oracle, frames)
    env = {"GSC_SCAN_DEBUG": "1"}
    if generic:
        env["GSC_SCAN_GENERIC"] = "1"
    got, err = run_child(tmp_path, frames, [("abi", "abi", list(frames))], env)
    for n in frames:
        assert want[n][2] == 100 if n == "nan" else want[n][2] < 100, n  # NaN rows: never converges (above)
        assert_matches_oracle(frame_result(got, "abi", n), want[n], (s, n))
    kinds = [("general", "0")] * 3 if generic else [("plain", str(want["plain"][2])), ("general", "0"), ("general", "0")]
    assert re.findall(r"kind (\w+) plain_passes (\d+)", err) == kinds, err[-1500:]
