"""yakmo seeding (gsc_yakmo.hip yakmo_seed2_kernel) against the oracle at small
shapes, step edges and odd data: labels equal, centroids equal as bit patterns
(the NaN rows of empty clusters included).  The cases and what each one makes
the kernel do are tests/yakmo_cases.py; test_yakmo_cases_host.py proves on the
CPU that every data kind reaches the mechanism it is here for.

Launch sites: `frames` is gsc_yakmo_seed_means_frames (one launch of one or
several frames, the body of gsc_yakmo_seed_means); `exports` is the reference
ABI yakmo_create(K,1,0,1,0,0,0) .. yakmo_train_on_data, once per stride.

What ran each path before this module (test_gpu_parity: two traced frames and
six synthetic shapes, N >= 3000, stride 8 / 16, K 256 .. 1024; test_gpu_abi:
one traced frame; the whole-file goldens), and what runs it here.  S is the
step: 1024 points at stride 8 / 16, 512 at 32.

  path                                           before                 here
  stride 32 (S = 512, chain_fast<8> only)        goldens cs9 .. cs16    every test, [32]
  colCount below the stride (zero-padded rows)   goldens                n_sweep: 2, 10, 18 columns
  N < 64, < S, at S, 2S, 3S (ring, prefetch      --                     n_sweep: 3 .. 6S + 7
    depth 3) and one past each
  last step of 8 full blocks + 5 (full <= 8      by chance              n_sweep: S + 517
    branch), of 9 full blocks (nbk = 9)          by chance              n_sweep: S + 576
  K = 1 (no chain), K = 2 (one chain)            --                     k_sweep
  K = 63 .. 65, 511 .. 513 (seed-table stride)   256, 512, 1024 only    k_sweep
  K = 1025, 4095, 4096 (cursor / sdlo union)     goldens cpf4096        k_sweep, dup to K 4096
  K = N - 1 (nearly every point chosen)          --                     k_sweep: N = K + 1, integer
  N = 262,144 (LDS) against 262,145 (HBM)        270,000 / 300,000      lds_boundary
  several frames, a different N and K each       goldens (one K)        frames_mixed
  HBM slices of neighbouring frames, n_off       --                     frames_mixed_big
    not a multiple of 32 / 64
  frame independent of its block index           --                     frames_repeat
  cum[] not partitioned by the target, probe     by chance              kinds: offset, dup, quiet_tail
    replay; lower_bound = N
  zero and negative totals, empty clusters       silence goldens        kinds: silence, dup, offset
  collision walk, its wrap at N - 1              --                     kinds: quiet_tail, dup
  skip share above 0.8, exact seed-distance ties --                     kinds: clusters, lattice
  ties on a total beyond 2^24 in the kernel      chain hook only        integer_wide
  non-finite totals                              --                     non_finite: overflow, nan
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import yakmo_cases as yc

pytestmark = pytest.mark.gpu

FP = ctypes.POINTER(ctypes.c_float)
IP = ctypes.POINTER(ctypes.c_int)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _diff(case, c, lab):
    """'' or what differs from the oracle run on this frame alone"""
    wc, wl = yc.want(case)
    bad = np.flatnonzero(np.asarray(lab) != wl)
    if bad.size:
        return f"{yc.case_id(case)}: {bad.size} labels differ, first at point {bad[0]} ({lab[bad[0]]} != {wl[bad[0]]})"
    rows = np.flatnonzero((_bits(c) != _bits(wc)).any(axis=1))
    if rows.size:
        return f"{yc.case_id(case)}: {rows.size} centroid rows differ in bits, first {rows[0]}"
    return ""


def frames(cases):
    """one launch of the cases' frames through gsc_yakmo_seed_means_frames"""
    import soundchunks_amd as sc

    cs, labs = sc.yakmo_seed_means_many([yc.data(c) for c in cases], [c.k for c in cases])
    return [(c, lab) for c, lab in zip(cs, labs)]


def exports(case):
    """the reference exports, as TFrame.Reduce calls them"""
    import soundchunks_amd as sc

    assert case.d in (8, 16, 32) and 0 < case.k < case.n  # they abort on anything else
    lib = sc.load()
    x = yc.data(case)
    rows = lambda a: (FP * a.shape[0])(*[ctypes.cast(a.ctypes.data + i * a.strides[0], FP)  # noqa: E731
                                         for i in range(a.shape[0])])
    y = lib.yakmo_create(case.k, 1, 0, 1, 0, 0, 0)
    assert y
    lib.yakmo_load_train_data(y, case.n, case.d, rows(x))
    lab = np.zeros(case.n, np.int32)
    lib.yakmo_train_on_data(y, lab.ctypes.data_as(IP))
    c = np.zeros((case.k, case.d), np.float32)
    lib.yakmo_get_centroids(y, rows(c))
    lib.yakmo_destroy(y)
    return c, lab


def check_singles(cases, through_exports=()):
    bad = [_diff(c, *frames([c])[0]) for c in cases]
    bad += [b + " (exports)" for b in (_diff(c, *exports(c)) for c in through_exports) if b]
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", ["gauss", "integer"])
@pytest.mark.parametrize("d", yc.STRIDES)
def test_n_sweep(d, kind):
    cases = yc.N_SWEEP[(d, kind)]
    s = yc.step_points(d)
    if kind == "gauss":
        check_singles(cases + [yc.SMALL_COLS[d]], through_exports=[c for c in cases if c.n == s + 1])
    else:
        check_singles(cases, through_exports=[c for c in cases if c.n == 3 * s])


@pytest.mark.parametrize("d", yc.STRIDES)
def test_k_sweep(d):
    cases = yc.K_SWEEP[d] + (yc.K_ALL_CHOSEN if d == 16 else [])
    check_singles(cases, through_exports=[c for c in cases if c.k == 513 and c.n == 514])


@pytest.mark.parametrize("d", yc.STRIDES)
def test_kinds(d):
    cases = [c for c in yc.KINDS[d] if c.kind not in ("overflow", "nan")]
    check_singles(cases + ([yc.INTEGER_WIDE] if d == 16 else []) + ([yc.DUP_MAX_K] if d == 8 else []))


@pytest.mark.parametrize("kind", ["overflow", "nan"])
@pytest.mark.parametrize("d", yc.STRIDES)
def test_non_finite(d, kind):
    check_singles([c for c in yc.KINDS[d] if c.kind == kind])


@pytest.mark.parametrize("d", [8, 32])
def test_lds_boundary(d):
    """262,144 points keep the bitmap and the prefix summaries in LDS, 262,145 in HBM"""
    cases = [c for c in yc.BOUNDARY if c.d == d]
    assert [c.n for c in cases] == [262144, 262145]
    check_singles(cases)


def check_launch(cases):
    bad = [b for b in (_diff(c, *got) for c, got in zip(cases, frames(cases))) if b]
    assert not bad, "\n".join(bad)


def test_frames_mixed():
    d, cases = yc.MIXED
    assert [(c.n, c.k) for c in cases] == [(65, 7), (1025, 33), (300, 299), (3073, 48), (64, 63)]
    check_launch(cases)


@pytest.mark.parametrize("group", ["big_first", "big_last"])
def test_frames_mixed_big(group):
    """one frame over 262,144 points: every frame of the launch runs the HBM instantiation"""
    d, cases = yc.MIXED_BIG_FIRST if group == "big_first" else yc.MIXED_BIG_LAST
    assert max(c.n for c in cases) == 262145
    check_launch(cases)


def test_frames_repeat():
    """the same three frames twice in one launch: a frame does not depend on its block index"""
    d, cases = yc.REPEAT
    got = frames(cases)
    for i in range(3):
        np.testing.assert_array_equal(got[i][1], got[i + 3][1])
        np.testing.assert_array_equal(_bits(got[i][0]), _bits(got[i + 3][0]))
    check_launch(cases)


def test_frames_entry_refuses_per_frame():
    import soundchunks_amd as sc

    x = yc.gen("gauss", 100, 16, 1)
    for fr, ks in (([x, x[:10]], [5, 10]), ([x[:10], x], [0, 5]), ([x], [100]), ([x, x], [5, 4097])):
        with pytest.raises(sc.GscError, match="0 < k < n"):
            sc.yakmo_seed_means_many(fr, ks)
    with pytest.raises(sc.GscError, match="features"):
        sc.yakmo_seed_means_many([np.zeros((100, 33), np.float32)], [5])
