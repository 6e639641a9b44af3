"""The ANN case matrix on the CPU (tests/ann_cases.py), before any of it runs
on a device: the oracle defines every case test_gpu_ann_matrix.py compares."""
from __future__ import annotations

import numpy as np

from ann_cases import FLT_MAX_BITS, FP, IP, err_bits, ora_tree_api, row_pointers, grid, nan_points


def test_oracle_defines_every_case(oracle):
    """on the CPU, before the device runs anything: the oracle ends and repeats
    itself on the NaN inputs, and past the n-th result it writes -1 / FLT_MAX"""
    ora = ora_tree_api(oracle)
    for n in (40, 1200):
        for row0 in (True, False):
            pts = nan_points(n, row0)
            assert np.isnan(pts[0]).any() == row0 and 0.04 < np.isnan(pts).any(axis=1).mean() < 0.08
            runs = []
            for rep in range(2):
                pa = row_pointers(pts)
                o = ora.ora_kdtree_create(pa, n, 8, 1)
                out = []
                rng = np.random.default_rng(5)
                for fn in (ora.ora_kdtree_search_multi, ora.ora_kdtree_pri_search_multi):
                    for k in (n, 3):
                        wi, we = np.zeros(k, np.int32), np.zeros(k, np.float32)
                        q = grid(rng, 1, 8)[0]
                        fn(o, wi.ctypes.data_as(IP), we.ctypes.data_as(FP), k, q.ctypes.data_as(FP), 0.0)
                        out += [wi.copy(), err_bits(we)]
                ora.ora_kdtree_destroy(o)
                runs.append(out)
            assert all((a == b).all() for a, b in zip(*runs))
            assert len(runs[0]) == 8 and (runs[0][0] >= -1).all() and (runs[0][0] < n).all()
    pts = grid(np.random.default_rng(1), 9, 8)
    pa = row_pointers(pts)
    o = ora.ora_kdtree_create(pa, 9, 8, 1)
    for fn in (ora.ora_kdtree_search_multi, ora.ora_kdtree_pri_search_multi):
        wi, we = np.zeros(12, np.int32), np.zeros(12, np.float32)
        fn(o, wi.ctypes.data_as(IP), we.ctypes.data_as(FP), 12, pts[0].ctypes.data_as(FP), 0.0)
        assert wi[9:].tolist() == [-1] * 3 and we.view(np.uint32)[9:].tolist() == [FLT_MAX_BITS] * 3
    ora.ora_kdtree_destroy(o)
