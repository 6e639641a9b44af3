"""The KNNFit case matrix on the CPU (tests/knnfit_cases.py): while at most 64
variants tie, the plain model of the reference rule gives the oracle's answer
(the premise knnfit_kernel stands on); and every case reaches the mechanism
it is in the matrix for: tie counts at the bucket edge, overflow counts, an
answer that depends on ANN's visiting order, tile multiples, denormal squares.

The conditions are conditions, not measurements: a seed that stops meeting one
is replaced in knnfit_cases, the threshold stays.
"""
from __future__ import annotations

import re

import numpy as np

import knnfit_cases as kc
import oracle_ffi

f32 = np.float32


def test_model_equals_oracle_up_to_the_bucket():
    """every case, every query with at most 64 ties; no answer is negative"""
    for c in kc.all_cases():
        best, cnt = kc.model(c)
        w = kc.want(c)
        fit = cnt <= kc.BUCKET
        np.testing.assert_array_equal(best[fit], w[fit], err_msg=kc.case_id(c))
        assert (w >= 0).all() and (w < 4 * c.r).all(), kc.case_id(c)
        assert cnt.min() >= 1


def test_matrix_is_covered():
    assert [c.cs for c in kc.CS_SWEEP] == list(range(1, 17))
    assert all((c.r, c.n) == (33, 257) for c in kc.CS_SWEEP)
    assert [(c.cs, c.r) for c in kc.R_EDGES] == [(cs, r) for cs in (8, 5) for r in (1, 2, 15, 16, 17)]
    assert len(kc.BUCKET_EDGES) == 12
    assert [c.n for c in kc.N_EDGES] == [1, 255, 256, 257, 513] and all(c.r == 40 for c in kc.N_EDGES)
    assert [c.arg for c in kc.SCALES] == [-60, -70, 10]
    assert [(c.r, c.n) for c in kc.MIXED] == [(1, 1), (17, 300), (2049, 64), (16, 257), (600, 513)]
    assert len({c.eps for c in kc.MIXED}) == 5 and len({c.cs for c in kc.MIXED}) == 1
    assert kc.REPEAT[:3] == kc.REPEAT[3:] and len(kc.REPEAT) == 6


def test_cs_sweep_queries_sit_on_and_near_every_variant():
    for c in kc.CS_SWEEP:
        fwd, q, eps = kc.data(c)
        assert len(np.unique(fwd, axis=0)) < c.r  # duplicates
        best, cnt = kc.model(c)
        if c.cs > 1:
            assert set((best % 4).tolist()) == {0, 1, 2, 3}, kc.case_id(c)
        assert (cnt > 1).any()


def test_r_edges_tie_every_variant():
    """4R = 60 and 64 fit the bucket, 68 does not"""
    for c in kc.R_EDGES:
        cnt = kc.model(c)[1]
        assert (cnt == 4 * c.r).all(), kc.case_id(c)
        assert kc.overflow(c) == (c.n if c.r == 17 else 0)


def test_bucket_edges_have_exactly_m_ties():
    for (m, way), c in kc.BUCKET_EDGES.items():
        fwd, q, eps = kc.data(c)
        best, cnt = kc.model(c)
        assert cnt[:4].tolist() == [m] * 4, kc.case_id(c)  # the queries on the four variants of the row
        assert (cnt[4:] < 60).all()
        assert (best[:4] % 4).tolist() == [0, 1, 2, 3]
        assert kc.overflow(c) == (4 if m > kc.BUCKET else 0)
        if way == "eps":
            assert eps > 0 and len(np.unique(fwd, axis=0)) == c.r  # no two copies equal
        else:
            assert eps == 0.0


def test_overflow_answers_depend_on_the_visiting_order():
    """at 65 and 66 copies placed by ORDER_SEED the oracle's answer is not the
    smallest tied index: a replay that ignored ANN's order would fail there"""
    for m in (65, 66):
        c = kc.BUCKET_EDGES[(m, "order")]
        best, cnt = kc.model(c)
        over = cnt > kc.BUCKET
        assert (kc.want(c)[over] != best[over]).any(), kc.case_id(c)
    c = kc.MIXED[1]
    best, cnt = kc.model(c)
    assert (cnt > kc.BUCKET).all() and (kc.want(c) != best).any()


def test_tile_edges_are_the_stated_multiples():
    for cs in kc.TILE_CS:
        t = 18432 // (cs + 1)
        assert kc.tile_rows(cs) == t
        assert [c.r for c in kc.TILE_EDGES[cs]] == [t - 1, t, t + 1, 2 * t + 1]
        for c in kc.TILE_EDGES[cs]:
            assert c.n == 64
            rows = set((kc.want(c) // 4).tolist())
            assert (kc.model(c)[1] == 1).all()  # each query has one nearest row and no tie
            # the first and the last row of every tile, and the one-row tail tile of t + 1 and 2t + 1
            expect = {p for p in (0, t - 1, t, 2 * t - 1, 2 * t, c.r - 1) if p < c.r}
            assert expect <= rows, (kc.case_id(c), sorted(rows))
            if c.r == t + 1:
                assert t in rows
            if c.r == 2 * t + 1:
                assert t in rows and 2 * t in rows
        for c in kc.TILE_TIES[cs]:
            fwd, q, eps = kc.data(c)
            same = np.flatnonzero((fwd == fwd[t + 1]).all(axis=1))
            assert same.tolist() == list(range(t - c.arg, t)) + [t + 1] and c.r == t + 2 and eps == 0.0
            assert kc.model(c)[1][:4].tolist() == [c.arg + 1] * 4  # c.arg ties in the first tile, one in the next
            assert kc.overflow(c) == (4 if c.arg == 64 else 0)
            if c.arg == 63:  # all in the bucket: the smallest tied row, in the first tile
                assert (kc.want(c)[:4] // 4 == t - 63).all()
    assert kc.tile_rows(8) == 2048 and kc.MIXED[2].r == kc.tile_rows(8) + 1


def test_frames_mixed_overflow_where_stated():
    assert [kc.overflow(c) > 0 for c in kc.MIXED] == [False, True, False, False, True]
    assert 4 * kc.MIXED[1].r == 68 and 4 * kc.MIXED[4].r == 2400 >= 512


def test_scale_cases_reach_denormals_and_vmax():
    for c in kc.SCALES[:2]:
        fwd, q, eps = kc.data(c)
        var = kc.variants(fwd)
        sq = (q[:, None, :] - var[None, :, :]) ** 2
        assert ((sq > 0) & (sq < kc.TINY)).any(), kc.case_id(c)
    # 2^-70: every square is denormal or zero, and so is every distance
    fwd, q, eps = kc.data(kc.SCALES[1])
    assert ((q[:, None, :] - kc.variants(fwd)[None, :, :]) ** 2 < kc.TINY).all()
    # a flush-to-zero build would answer this case differently
    assert (kc.model(kc.SCALES[1], ftz=True)[0] != kc.model(kc.SCALES[1])[0]).any()
    fwd, q, eps = kc.data(kc.SCALES[2])
    assert np.abs(fwd).max() > 1000
    fwd, q, eps = kc.data(kc.BIG_CAND)
    vv = (fwd.astype(np.float64) ** 2).sum(axis=1)
    assert vv.max() >= 2.0 ** 20 * np.median(vv)
    fwd, q, eps = kc.data(kc.BIG_QUERY)
    qq = (q.astype(np.float64) ** 2).sum(axis=1)
    assert (qq > 2.0 ** 60).sum() == 1 and np.isfinite(f32(qq.max() * 4))


def test_oracle_does_not_flush_denormals():
    """oracle/Makefile builds without -ffast-math (whose start-up code sets
    flush-to-zero for the whole process), denormal float32 arithmetic survives
    in this process with the oracle loaded, and the oracle answers the 2^-70
    case like the unflushed model, not like the flushed one"""
    mk = (oracle_ffi.ORACLE_DIR / "Makefile").read_text()
    flags = re.search(r"^CFLAGS \?= (.*)$", mk, re.M).group(1).split()
    assert "-fno-fast-math" in flags
    assert not {"-ffast-math", "-Ofast", "-funsafe-math-optimizations", "-mdaz-ftz"} & set(flags)
    oracle_ffi.load()
    a = f32(2.0) ** f32(-70)
    assert a * a > 0 and a * a == f32(2.0) ** f32(-140)
    c = kc.SCALES[1]
    np.testing.assert_array_equal(kc.want(c), kc.model(c)[0])
    assert (kc.want(c) != kc.model(c, ftz=True)[0]).any()


def test_gap_cases_sit_on_the_decision_boundary():
    """eps one ulp below the gap keeps the nearest row, eps at the gap takes the
    smaller index: an inexact sqrt on either side flips the answer"""
    flips = 0
    for cs, cases in kc.GAPS.items():
        for i in range(0, len(cases), 3):
            below, at, above = (int(kc.want(c)[0]) for c in cases[i:i + 3])
            assert at < 4 and above < 4
            flips += below >= 4
    assert flips >= 40
    assert kc.want(kc.IEEE_SQRT).tolist() == [2]
