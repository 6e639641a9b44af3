"""KNNFit (gsc_kernels.hip knnfit_kernel, and the overflow replay: gsc_ann.hip
build_many_kernel + knnfit_ann_kernel) against the oracle at small shapes and
edges: every case goes through gsc_knnfit_assign_frames (one launch of one or
several frames, the body of gsc_knnfit_assign); `best` equals the oracle run on
that frame alone and `overflow` equals the model's count of queries with more
than 64 ties.  The cases are tests/knnfit_cases.py; test_knnfit_cases_host.py
proves on the CPU that each one reaches the mechanism it is here for.

What ran each path before this module (test_gpu_parity: three traced frames,
four synthetic shapes at CS 4 / 8 / 16 with N 1500 .. 3000, one sqrt query and
an eps sweep over two-row frames; test_gpu_signal_edges; the whole-file
goldens), and what runs it here.  t = 18432 // (CS + 1) is the candidate tile.

  path                                           before                 here
  knnfit_kernel<CS>, 16 instantiations           CS 4, 8, 16; the rest  cs_sweep: CS 1 .. 16
                                                   in goldens only
  4R below, at, above the bucket (R 15, 16, 17)  --                     r_edges (and R = 1, 2)
  tie count 63, 64, 65, 66 (cnt > 64)            thousands of ties      bucket_edges: eps = 0, perturbed
                                                                          copies within eps, copies whose
                                                                          smallest index ANN meets last
  R = t - 1 (tile clipped to R), t, t + 1 and    R = 4096 at CS 8       tile_edges at CS 8, 15, 16: nearest
    2t + 1 (one-row tail tiles)                    by chance              row first / last / alone in a tile;
                                                                          64 + 1 and 63 + 1 ties across the edge
  N = 1, 255, 256, 257, 513 (query tile of 256)  N 1500 .. 3000         n_edges
  idle blocks (ti * 256 >= N)                    --                     frames_mixed: N = 1 beside N = 513
  the bound eb = (qq + vmax) 2^-17 away from     --                     scales: data x 2^-60, 2^-70, 2^10,
    scale 1; denormal squares                                             one candidate x 2^12, one huge query
  eps on the decision boundary (IEEE sqrt)       parity: 24 pairs       eps_gap: 48 pairs x 3 eps, one launch
                                                                          per CS; the traced sqrt frame
  several frames in one launch, an R, N and eps  whole files only       frames_mixed, both orders
    each; build_many with a 68-point and a
    2400-point tree (lane and wave levels)
  frame independent of its block index           --                     frames_repeat
  the entry's argument checks                    --                     refusals
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import knnfit_cases as kc

pytestmark = pytest.mark.gpu


def launch(cases):
    """one launch of the cases' frames: [(best, overflow count)]"""
    import soundchunks_amd as sc

    d = [kc.data(c) for c in cases]
    best, ov = sc.knnfit_assign_many([x[0] for x in d], [x[1] for x in d], [x[2] for x in d])
    return list(zip(best, ov))


def _diff(case, best, ov):
    """'' or what differs from the oracle run on this frame alone"""
    w = kc.want(case)
    bad = np.flatnonzero(np.asarray(best) != w)
    if bad.size:
        return (f"{kc.case_id(case)}: {bad.size} of {len(w)} answers differ, first at query {bad[0]} "
                f"({best[bad[0]]} != {w[bad[0]]}, {kc.model(case)[1][bad[0]]} ties)")
    if ov != kc.overflow(case):
        return f"{kc.case_id(case)}: overflow {ov} != {kc.overflow(case)}"
    return ""


def check_singles(cases):
    bad = [b for b in (_diff(c, *launch([c])[0]) for c in cases) if b]
    assert not bad, "\n".join(bad)


def check_launch(cases):
    bad = [b for b in (_diff(c, *got) for c, got in zip(cases, launch(cases))) if b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cs", range(1, 17))
def test_cs_sweep(cs):
    check_singles([kc.CS_SWEEP[cs - 1]])


@pytest.mark.parametrize("cs", [8, 5])
def test_r_edges(cs):
    cases = [c for c in kc.R_EDGES if c.cs == cs]
    assert [4 * c.r for c in cases] == [4, 8, 60, 64, 68]
    check_singles(cases)


@pytest.mark.parametrize("way", kc.BUCKET_WAYS)
@pytest.mark.parametrize("m", kc.BUCKET_M)
def test_bucket_edges(m, way):
    check_singles([kc.BUCKET_EDGES[(m, way)]])


@pytest.mark.parametrize("cs", kc.TILE_CS)
def test_tile_edges(cs):
    check_singles(kc.TILE_EDGES[cs] + kc.TILE_TIES[cs])


def test_n_edges():
    check_singles(kc.N_EDGES)


@pytest.mark.parametrize("p", [-60, -70, 10])
def test_scales(p):
    check_singles([c for c in kc.SCALES if c.arg == p])


def test_scales_one_big_candidate():
    check_singles([kc.BIG_CAND])


def test_scales_one_big_query():
    check_singles([kc.BIG_QUERY])


@pytest.mark.parametrize("cs", sorted(kc.GAPS))
def test_eps_gap(cs):
    """eps one ulp below, at and above the f32 gap of 16 two-row frames, one launch"""
    check_launch(kc.GAPS[cs])


def test_eps_tie_needs_ieee_sqrt():
    check_singles([kc.IEEE_SQRT])


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_frames_mixed(order):
    cases = kc.MIXED if order == "forward" else kc.MIXED[::-1]
    check_launch(cases)


def test_frames_repeat():
    """the same three frames twice in one launch: a frame does not depend on its block index"""
    got = launch(kc.REPEAT)
    for i in range(3):
        np.testing.assert_array_equal(got[i][0], got[i + 3][0])
        assert got[i][1] == got[i + 3][1]
    check_launch(kc.REPEAT)


def test_single_frame_entry_is_the_frames_entry():
    import soundchunks_amd as sc

    for c in (kc.R_EDGES[4], kc.CS_SWEEP[2]):
        fwd, q, eps = kc.data(c)
        np.testing.assert_array_equal(sc.knnfit_assign(fwd, q, eps), kc.want(c))


def test_refusals():
    import soundchunks_amd as sc

    lib = sc.load()
    FP, IP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    fwd, q, eps = kc.data(kc.R_EDGES[1])
    one = lambda v, t: np.array([v], t)  # noqa: E731
    ok = dict(nf=1, cs=8, rs=one(2, np.int32), cand=np.array(fwd), ns=one(40, np.int32), q=np.array(q),
              eps=one(eps, np.float32), best=np.zeros(40, np.int32), ov=np.zeros(1, np.int32))

    def call(**kw):
        a = {**ok, **kw}
        p = lambda x, t: None if x is None else x.ctypes.data_as(t)  # noqa: E731
        return lib.gsc_knnfit_assign_frames(a["nf"], a["cs"], p(a["rs"], IP), p(a["cand"], FP), p(a["ns"], IP),
                                            p(a["q"], FP), p(a["eps"], FP), p(a["best"], IP), p(a["ov"], IP))

    def refused(match, **kw):
        assert call(**kw) != 0
        msg = lib.gsc_last_error().decode()
        assert "gsc_knnfit_assign_frames" in msg and match in msg, msg

    assert call() == 0 and call(ov=None) == 0  # overflow may be null
    np.testing.assert_array_equal(ok["best"], kc.want(kc.R_EDGES[1]))
    refused("nf", nf=0)
    refused("nf", nf=-1)
    refused("cs", cs=0)
    refused("cs", cs=17)
    refused("every r", rs=one(0, np.int32))
    refused("every n", ns=one(0, np.int32))
    for name, key in (("rs", "rs"), ("cand_fwd", "cand"), ("ns", "ns"), ("q", "q"), ("eps", "eps"), ("best", "best")):
        refused(f"{name} is null", **{key: None})
    with pytest.raises(sc.GscError, match="every r"):
        sc.knnfit_assign_many([fwd, fwd[:0]], [q, q], [0.0, 0.0])
