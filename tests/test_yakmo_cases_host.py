"""The yakmo case matrix on the CPU (tests/yakmo_cases.py): the path model
gives the oracle's labels on every case, so its statistics describe what the
oracle (and a kernel that equals it) does on that input; every data kind
reaches the mechanism it is in the matrix for; and the kernel's Elkan bound,
replayed on the model's distances, never skips a point the reference improves.

The conditions are conditions, not measurements: a seed that stops meeting one
is replaced in yakmo_cases.KIND_SEEDS, the threshold stays.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import yakmo_cases as yc


@functools.lru_cache(maxsize=None)
def _model(case):
    return yc.model(yc.data(case), case.k)


def _check(cases):
    for c in cases:
        lab, st = _model(c)
        np.testing.assert_array_equal(lab, yc.want(c)[1], err_msg=yc.case_id(c))
        assert st["unsound"] == 0, (yc.case_id(c), st)


@pytest.mark.parametrize("d", yc.STRIDES)
def test_model_equals_oracle_n_sweep(d):
    _check(yc.N_SWEEP[(d, "gauss")] + yc.N_SWEEP[(d, "integer")] + [yc.SMALL_COLS[d]])


@pytest.mark.parametrize("d", yc.STRIDES)
def test_model_equals_oracle_k_sweep(d):
    _check(yc.K_SWEEP[d] + (yc.K_ALL_CHOSEN if d == 16 else []))


@pytest.mark.parametrize("d", yc.STRIDES)
def test_model_equals_oracle_kinds(d):
    _check(yc.KINDS[d] + ([yc.INTEGER_WIDE] if d == 16 else []) + ([yc.DUP_MAX_K] if d == 8 else []))


def test_model_equals_oracle_boundary_and_frames():
    _check(yc.BOUNDARY + yc.MIXED[1] + yc.MIXED_BIG_FIRST[1] + yc.MIXED_BIG_LAST[1] + yc.REPEAT[1])


def test_matrix_is_covered():
    """the four tests above ran every case of the matrix"""
    groups = [yc.N_SWEEP[(d, k)] for d in yc.STRIDES for k in ("gauss", "integer")]
    assert list(map(len, groups)) == [15] * 6
    assert {d: c.d for d, c in yc.SMALL_COLS.items()} == {8: 2, 16: 10, 32: 18}
    assert len(yc.K_SWEEP[16]) == 24 and len(yc.K_SWEEP[8]) == len(yc.K_SWEEP[32]) == 8


def _kind(kind, d):
    (c,) = [c for c in yc.KINDS[d] if c.kind == kind]
    return c, _model(c)[1]


@pytest.mark.parametrize("d", yc.STRIDES)
def test_kind_conditions(d):
    c, st = _kind("silence", d)
    assert (c.n, c.k) == (130, 7)
    assert st["zero_total"] == c.k - 1 and st["empty"] == c.k - 1 and st["walk_steps"] > 0

    c, st = _kind("signed_zero", d)
    x = yc.data(c)
    assert not x[:c.n - 50].any() and np.signbit(x[0]).all() and not np.signbit(x[1]).any()
    assert st["first_total"] > 0 and st["nonfinite_total"] == 0

    c, st = _kind("quiet_tail", d)
    assert (c.n, c.k) == (200, 9) and st["wraps"] >= 1

    c, st = _kind("dup", d)
    assert c.k == 40 and st["nonpart"] >= 1 and st["neg_total"] >= 1 and st["lb_n"] >= 1
    assert st["empty"] == c.k - 5 and st["skip_share"] > 0.5

    c, st = _kind("offset", d)
    assert st["nonpart"] > c.k / 2 and st["neg_d0"] > c.n / 2

    for kind in ("clusters", "lattice"):
        c, st = _kind(kind, d)
        assert st["skip_share"] > 0.8 and st["unsound"] == 0

    c, st = _kind("overflow", d)
    x = yc.data(c).astype(np.float64)
    assert np.isfinite((x * x).sum(axis=1).astype(np.float32)).all()  # finite rows and norms
    assert st["nonfinite_total"] >= 1 and st["unsound"] == 0

    c, st = _kind("nan", d)
    assert np.isnan(yc.data(c)).sum() == 1 and st["nonfinite_total"] >= 1

    for kind in ("cep", "outliers"):
        c, st = _kind(kind, d)
        assert 700 <= c.n <= 3100 and 16 <= c.k <= 64


def test_integer_wide_conditions():
    st = _model(yc.INTEGER_WIDE)[1]
    assert st["first_total"] >= 2.0 ** 24 and st["ties"] >= 100


def test_dup_to_max_k_conditions():
    c = yc.DUP_MAX_K
    st = _model(c)[1]
    assert (c.n, c.d, c.k) == (4200, 8, 4096)
    assert st["walk_steps"] > 10 ** 6
    assert st["nonpart"] >= 1 and st["neg_total"] >= 1 and st["lb_n"] >= 1
    assert st["empty"] == c.k - 5 and st["skip_share"] > 0.5


def test_n_sweep_reaches_the_chain_branches():
    """At stride 8 / 16 a last step of S + 517 points has eight full blocks (the
    full <= 8 branch to chain_fast<8>), S + 576 nine (nbk = 9 on 16 points per lane)."""
    for d in yc.STRIDES:
        s = yc.step_points(d)
        ns = yc.n_sweep(d)
        assert (ns[7] - s) >> 6 == 8 and (ns[7] - s) & 63 == 5 and (ns[8] - s) >> 6 == 9
        assert all(c.k == min(c.n - 1, 48) for c in yc.N_SWEEP[(d, "gauss")])
