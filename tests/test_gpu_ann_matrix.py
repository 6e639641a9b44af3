"""The ANN drop-in exports (gsc_abi.cpp over gsc_ann.hip build_kernel and
query_kernel: ann_kdtree_create / _search / _pri_search / _search_multi /
_pri_search_multi / _destroy) against the oracle's ora_kdtree_* at small
shapes and edges: indices equal, errors equal as bit patterns (a NaN error is
compared as NaN: its payload is not part of the reference's contract).

The tree is not exported, so the build is observed through searches with
k = n: both searches then list every point, and points at equal distance come
in the order the search visits the leaves -- the order annMedianSplit's swaps
left them in.

What ran each path before this module (test_gpu_abi: n = 32, 300, 3000 and the
traced frame's 4R candidates, dd = 8 / 16, eps = 0, k <= 64 < n), and here:

  path                                           before            here
  build: n = 1 (no split), 2, 3, 5               --                n_sweep
  build: n = 63 .. 65, not a power of two        300, 3000         n_sweep
  build: root on the lane path (511) and on the  3000 only         n_sweep: 511, 512, 513, 1023, 1025
    wave path (512 = kWaveSeg)
  build: dd = 1, 3, 16, 32                       dd 8 (16: frame)  n_sweep at n = 513, 1025
  build: zero spread, quickselect on equal keys  --                all_equal
  build: NaN rows, lane path and wave path, the  --                nan_rows
    "a NaN first value never moves" rule
  leaf order among ties                          k <= 64           k = n in every case above
  search: k = n - 1, n, k > n (-1 / FLT_MAX)     --                k_edges
  search: eps > 0 (max_err), both searches       0.0 only          eps
  stale tree, live rows                          n 300, 3000 dd 8  stale: n = 513, dd = 16

Nothing is left out: the oracle terminates and is deterministic on every NaN
input here and writes -1 / FLT_MAX past the n-th result (checked on the CPU
by test_ann_cases_host.py, without a device).

The exports abort the process on misuse (the reference ABI has no error
channel), so every call here passes a live handle and a valid shape.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from ann_cases import FLT_MAX_BITS, FP, IP, err_bits, ora_tree_api, row_pointers, grid, nan_points

pytestmark = pytest.mark.gpu


class Pair:
    """the same rows under our tree and the oracle's"""

    def __init__(self, oracle, pts):
        import soundchunks_amd as sc

        self.lib, self.ora, self.pts = sc.load(), ora_tree_api(oracle), pts
        self.pa = row_pointers(pts)  # both trees keep the row pointers: alive as long as the trees
        n, dd = pts.shape
        self.t = self.lib.ann_kdtree_create(self.pa, n, dd, 1, 0)
        self.o = self.ora.ora_kdtree_create(self.pa, n, dd, 1)
        assert self.t and self.o

    def close(self):
        self.lib.ann_kdtree_destroy(self.t)
        self.ora.ora_kdtree_destroy(self.o)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def multi(self, q, k, eps=0.0, modes=("search", "pri")):
        q = np.ascontiguousarray(q, dtype=np.float32)
        qp = q.ctypes.data_as(FP)
        for mode in modes:
            ours = self.lib.ann_kdtree_search_multi if mode == "search" else self.lib.ann_kdtree_pri_search_multi
            theirs = self.ora.ora_kdtree_search_multi if mode == "search" else self.ora.ora_kdtree_pri_search_multi
            gi, ge = np.full(k, -7, np.int32), np.full(k, -7, np.float32)
            wi, we = np.full(k, -9, np.int32), np.full(k, -9, np.float32)
            ours(self.t, gi.ctypes.data_as(IP), ge.ctypes.data_as(FP), k, qp, eps)
            theirs(self.o, wi.ctypes.data_as(IP), we.ctypes.data_as(FP), k, qp, eps)
            what = f"{mode} n={self.pts.shape[0]} dd={self.pts.shape[1]} k={k} eps={eps}"
            np.testing.assert_array_equal(gi, wi, err_msg=what)
            np.testing.assert_array_equal(err_bits(ge), err_bits(we), err_msg=what)
        return wi, we

    def single(self, q, eps=0.0):
        """ann_kdtree_search and ann_kdtree_pri_search (k = 1, the index returned)"""
        q = np.ascontiguousarray(q, dtype=np.float32)
        qp = q.ctypes.data_as(FP)
        ge, we = ctypes.c_float(), ctypes.c_float()
        assert self.lib.ann_kdtree_search(self.t, qp, eps, ctypes.byref(ge)) == \
            self.ora.ora_kdtree_search(self.o, qp, eps, ctypes.byref(we))
        assert err_bits(np.float32(ge.value)[None]) == err_bits(np.float32(we.value)[None])
        wi, wv = np.zeros(1, np.int32), np.zeros(1, np.float32)
        self.ora.ora_kdtree_pri_search_multi(self.o, wi.ctypes.data_as(IP), wv.ctypes.data_as(FP), 1, qp, eps)
        assert self.lib.ann_kdtree_pri_search(self.t, qp, eps, ctypes.byref(ge)) == wi[0]
        assert err_bits(np.float32(ge.value)[None]) == err_bits(wv)


def sweep(p, rng, queries, full):
    """`full` searches with k = n (the leaf order), `queries` with k = 1 and 7, on and off the grid points"""
    n, dd = p.pts.shape
    finite = p.pts[np.isfinite(p.pts).all(axis=1)]
    for i in range(full):
        p.multi(finite[rng.integers(0, len(finite))] if i % 2 == 0 else grid(rng, 1, dd)[0], n)
    for i in range(queries):
        q = finite[rng.integers(0, len(finite))] if i % 3 == 0 else grid(rng, 1, dd)[0]
        p.multi(q, 1)
        p.multi(q, min(7, n))
        if i < 4:
            p.single(q)


N_SWEEP = [(n, 8) for n in (1, 2, 3, 5, 63, 64, 65, 511, 512, 513, 1023, 1025)] + \
          [(n, dd) for dd in (1, 3, 16, 32) for n in (513, 1025)]


@pytest.mark.parametrize("n,dd", N_SWEEP)
def test_n_sweep(oracle, n, dd):
    rng = np.random.default_rng([3, n, dd])
    with Pair(oracle, grid(rng, n, dd)) as p:
        big = n > 100
        sweep(p, rng, queries=8 if big else 12, full=2 if big else 6)


@pytest.mark.parametrize("n", [7, 64, 600])
def test_all_equal(oracle, n):
    """zero spread in every dimension: cdim stays 0 and the quickselect runs over equal keys"""
    rng = np.random.default_rng(n)
    pts = np.ascontiguousarray(np.repeat(grid(rng, 1, 8), n, axis=0))
    with Pair(oracle, pts) as p:
        wi, we = p.multi(pts[0], n)
        assert len(set(we.tolist())) == 1 and sorted(wi.tolist()) == list(range(n))
        p.multi(grid(rng, 1, 8)[0], n)
        sweep(p, rng, queries=4, full=0)


@pytest.mark.parametrize("row0_nan", [True, False])
@pytest.mark.parametrize("n", [40, 1200])
def test_nan_rows(oracle, n, row0_nan):
    """about 5 % NaN rows; n = 1200 builds its first two levels on the wave path"""
    pts = nan_points(n, row0_nan)
    rng = np.random.default_rng(n)
    with Pair(oracle, pts) as p:
        for i in range(2 if n > 100 else 6):
            p.multi(grid(rng, 1, 8)[0], n, modes=("search", "pri"))
        for i in range(8):
            q = grid(rng, 1, 8)[0]
            p.multi(q, 3)
            p.single(q)


@pytest.mark.parametrize("n", [9, 70])
def test_k_edges(oracle, n):
    rng = np.random.default_rng(n)
    with Pair(oracle, grid(rng, n, 8)) as p:
        for k in (1, 2, n - 1, n, n + 3):
            for i in range(4):
                wi, we = p.multi(p.pts[rng.integers(0, n)] if i % 2 else grid(rng, 1, 8)[0], k)
                if k > n:  # what the oracle writes past the n-th result
                    assert wi[n:].tolist() == [-1] * 3 and we.view(np.uint32)[n:].tolist() == [FLT_MAX_BITS] * 3


@pytest.mark.parametrize("eps", [0.5, 3.0])
@pytest.mark.parametrize("n", [300, 1025])
def test_eps(oracle, n, eps):
    """max_err = (1 + eps)^2 prunes both searches: the answers are approximate, and the same"""
    rng = np.random.default_rng([n, int(eps * 2)])
    pts = np.ascontiguousarray(rng.normal(size=(n, 8)), dtype=np.float32)
    pruned = 0
    with Pair(oracle, pts) as p:
        for i in range(14):
            q = rng.normal(size=8).astype(np.float32)
            for k in (1, 7):
                wi, we = p.multi(q, k, eps)
                d = np.sort(((pts.astype(np.float64) - q) ** 2).sum(axis=1))[:k]
                pruned += int((we.astype(np.float64) > d * (1 + 1e-5)).any())
            p.single(q, eps)
    assert pruned > 0  # eps did cut a branch that held a nearer point


def test_stale(oracle):
    """the stale-tree protocol of test_gpu_abi at n = 513, dd = 16: points move in place, the trees stay"""
    rng = np.random.default_rng(513)
    pts = grid(rng, 513, 16)
    with Pair(oracle, pts) as p:
        for step in range(20):
            q = grid(rng, 1, 16)[0]
            p.multi(q, 1)
            p.multi(q, 7)
            if step % 10 == 0:
                p.multi(q, 513)
            p.single(q)
            pts[rng.integers(0, 513)] += np.float32(0.25)
