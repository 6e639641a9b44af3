"""Shared by test_ann_cases_host.py and test_gpu_ann_matrix.py: ctypes access to
the oracle's kd-tree, the point generators, the comparison of error bits.

Plain module: no fixtures, no GPU.
"""
from __future__ import annotations

import ctypes

import numpy as np

FP = ctypes.POINTER(ctypes.c_float)
IP = ctypes.POINTER(ctypes.c_int)
FLT_MAX_BITS = 0x7F7FFFFF
QNAN = 0x7FC00000


def row_pointers(a):
    return (FP * a.shape[0])(*[ctypes.cast(a.ctypes.data + i * a.strides[0], FP) for i in range(a.shape[0])])


def ora_tree_api(oracle):
    lib = oracle.load()
    lib.ora_kdtree_create.restype = ctypes.c_void_p
    lib.ora_kdtree_create.argtypes = [ctypes.POINTER(FP), ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.ora_kdtree_destroy.argtypes = [ctypes.c_void_p]
    for fn in (lib.ora_kdtree_search_multi, lib.ora_kdtree_pri_search_multi):
        fn.argtypes = [ctypes.c_void_p, IP, FP, ctypes.c_int, FP, ctypes.c_float]
    lib.ora_kdtree_search.argtypes = [ctypes.c_void_p, FP, ctypes.c_float, FP]
    lib.ora_kdtree_search.restype = ctypes.c_int
    return lib


def err_bits(e):
    b = np.ascontiguousarray(e).view(np.uint32).copy()
    b[np.isnan(e)] = QNAN
    return b


def grid(rng, n, dd):
    """coarse grid: exact ties in every distance and every cut value"""
    return np.ascontiguousarray(np.round(rng.normal(size=(n, dd)) * 8) / 8, dtype=np.float32)


def nan_points(n, row0_nan):
    rng = np.random.default_rng([11, n, int(row0_nan)])
    pts = grid(rng, n, 8)
    bad = rng.choice(np.arange(1, n), max(2, n // 20), replace=False)
    pts[bad, rng.integers(0, 8, size=len(bad))] = np.nan  # one NaN coordinate each
    pts[bad[0]] = np.nan  # and one row NaN in every coordinate
    if row0_nan:
        pts[0, 3] = np.nan
    return pts
