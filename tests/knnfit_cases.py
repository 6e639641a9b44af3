"""Inputs for KNNFit (gsc_kernels.hip knnfit_kernel, the overflow replay of
gsc_ann.hip knnfit_ann_kernel) and a plain model of the reference rule.

  data(case)    (forward rows R x CS, queries N x CS, eps): deterministic
  want(case)    oracle.knnfit_assign on that frame alone, cached by case
  model(case)   the rule restated in numpy float32, per query: the smallest
                tied index and the tie count
                  e_f = sequential float32 sum over j of (q_j - v_fj)^2 for the
                        4R variants f = 4c + 2neg + rev
                  s_f = sqrt(e_f / CS) in float32
                  tied: |s_f - s_min| <= eps
                While at most 64 variants tie, all of them sit in ANN's 64-NN
                bucket (acceptance is monotone in e) and the oracle's answer
                is the smallest tied index: the premise knnfit_kernel stands
                on.  Beyond 64 the bucket holds the first 64 that ANN's
                priority search meets and only the oracle knows the answer.
  the matrix    shared by test_knnfit_cases_host.py (every case reaches the
                mechanism it is here for) and test_gpu_knnfit_matrix.py (the
                kernels equal the oracle)

Domain: finite values whose squared distances stay finite.  NaN and infinity
never reach KNNFit (the candidates are dequantised int16, the queries come
from finite PCM), so no case holds one.

Plain module: no fixtures, no GPU.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

f32 = np.float32
BUCKET = 64  # CBucketSize (encoder.lpr:917)

# kind: the generator; arg: what that generator needs beyond the shape
Case = namedtuple("Case", "kind cs r n eps arg seed")


def tile_rows(cs):
    """candidate rows of one LDS tile (72 KB of values + |v|^2)"""
    return 18432 // (cs + 1)


def _quantised(rng, r, cs):
    """8-bit-quantised rows, about half of them duplicates"""
    base = np.round(rng.uniform(-1, 1, size=(max(1, r // 2), cs)) * 127) / 127
    fwd = np.concatenate([base, base[rng.integers(0, len(base), size=r - len(base))]]).astype(f32)
    rng.shuffle(fwd)
    return fwd


def _variant(rows, flip):
    """rows as variant flip (bit 0: reversed, bit 1: negated)"""
    flip = np.asarray(flip)
    out = np.where((flip & 1)[:, None] == 1, rows[:, ::-1], rows)
    return out * np.where(flip >= 2, f32(-1.0), f32(1.0))[:, None]


def _near(rng, fwd, n, noise=0.002):
    """queries on (30 %) or near (70 %) every variant of random rows"""
    pick = _variant(fwd[rng.integers(0, len(fwd), size=n)], np.arange(n) % 4)
    nz = rng.normal(0, noise, size=pick.shape) * (rng.uniform(size=(n, 1)) < 0.7)
    return (pick + nz).astype(f32)


def _asym(rng, cs):
    """a row none of whose variants equals another (for cs >= 2)"""
    return (np.arange(1, cs + 1) / f32(cs + 1) * f32(0.5) + rng.uniform(0.05, 0.1)).astype(f32)


# the frame of test_knnfit_eps_tie_needs_ieee_sqrt: |s1 - s0| lands 0.3 ulp below eps
_IEEE = (np.array([[0x3d8be665, 0x3d8f274a, 0x3d503926, 0x3dbff4af, 0x3e12682f, 0x3e1408a1, 0x3e1dcb4f, 0x3e467678],
                   [0x3d281020, 0x3d5c3871, 0x3d566cda, 0x3e0f6ede, 0x3e1254a9, 0x3e199326, 0x3dfefdfc, 0x3e2af5ec]],
                  np.uint32),
         np.array([[0xbd5ae1b6, 0xbd86810d, 0xbd95b12b, 0xbdfb71f7, 0xbe02d106, 0xbe012902, 0xbe1a3134, 0xbe2ec15e]],
                  np.uint32), 0x3a24b306)


TINY = f32(2.0) ** f32(-126)  # the smallest normal float32


def _seq_s(q, var, ftz=False):
    """s_f of one query against the rows of var, sequential float32; ftz: what
    a flush-to-zero build would compute (denormal squares and sums become 0)"""
    flush = (lambda a: np.where(np.abs(a) < TINY, f32(0), a)) if ftz else (lambda a: a)
    e = np.zeros(len(var), f32)
    for j in range(var.shape[1]):
        t = q[j] - var[:, j]
        e = flush(e + flush(t * t))
    return np.sqrt(flush(e / f32(var.shape[1])))


def variants(fwd):
    v = np.empty((4 * len(fwd), fwd.shape[1]), f32)
    v[0::4], v[1::4], v[2::4], v[3::4] = fwd, fwd[:, ::-1], -fwd, -fwd[:, ::-1]
    return v


@functools.lru_cache(maxsize=None)
def data(case):
    """(fwd, q, eps) of a case; the arrays are read-only"""
    c = case
    rng = np.random.default_rng([c.seed, c.cs, c.r, c.n])
    eps = f32(c.eps)
    if c.kind == "sweep":  # arg: power-of-two scale of the data and of eps
        fwd = _quantised(rng, c.r, c.cs)
        q = _near(rng, fwd, c.n)
        k = f32(2.0) ** f32(c.arg)
        fwd, q, eps = fwd * k, q * k, f32(eps * k)
    elif c.kind == "bucket":  # arg: (m copies, way)
        m, way = c.arg
        row = _asym(rng, c.cs)
        fwd = rng.uniform(-1, 1, size=(c.r, c.cs)).astype(f32)
        at = np.sort(rng.choice(c.r, m, replace=False))
        fwd[at] = row
        if way == "eps":  # perturbed copies, all within eps of the query's nearest
            fwd[at] += rng.uniform(-1e-4, 1e-4, size=(m, c.cs)).astype(f32)
        q = np.concatenate([_variant(np.repeat(row[None], 4, 0), np.arange(4)),
                            _near(rng, np.delete(fwd, at, axis=0), c.n - 4)]).astype(f32)
    elif c.kind == "tile":  # the nearest row first / last in a tile, or the tile's only row
        t = tile_rows(c.cs)
        fwd = rng.uniform(-1, 1, size=(c.r, c.cs)).astype(f32)
        spots = [p for p in (0, t - 1, t, 2 * t - 1, 2 * t, c.r - 1) if p < c.r]
        pos = np.array([spots[i % len(spots)] for i in range(c.n)])
        q = _variant(fwd[pos], (np.arange(c.n) // len(spots)) % 4)
        q = (q + rng.normal(0, 1e-3, size=q.shape) * (np.arange(c.n)[:, None] % 3 > 0)).astype(f32)
    elif c.kind == "tiletie":  # arg m: m copies of one row end the first tile, one more sits in the next
        t = tile_rows(c.cs)
        assert c.r == t + 2
        fwd = rng.uniform(-1, 1, size=(c.r, c.cs)).astype(f32)
        row = _asym(rng, c.cs)
        fwd[t - c.arg:t] = row
        fwd[t + 1] = row
        q = np.concatenate([_variant(np.repeat(row[None], 4, 0), np.arange(4)),
                            _near(rng, fwd[:8], c.n - 4)]).astype(f32)
    elif c.kind == "bigcand":  # one candidate 2^12 times the rest: vmax is all its
        fwd = _quantised(rng, c.r, c.cs)
        q = _near(rng, fwd, c.n)
        fwd[c.r // 2] = _asym(rng, c.cs) * f32(4096.0)
    elif c.kind == "bigquery":  # one huge query among ordinary ones
        fwd = _quantised(rng, c.r, c.cs)
        q = _near(rng, fwd, c.n)
        q[c.n // 2] *= f32(2.0 ** 40)
    elif c.kind == "copies":  # arg: m equal rows in a frame of ordinary ones
        fwd = _quantised(rng, c.r, c.cs)
        row = _asym(rng, c.cs)
        fwd[rng.choice(c.r, c.arg, replace=False)] = row
        q = _near(rng, fwd, c.n)
        q[:8] = _variant(np.repeat(row[None], 8, 0), np.arange(8) % 4)
    elif c.kind == "gap":  # eps one ulp below (arg -1), at (0), above (1) the f32 gap s1 - s0
        while True:
            fwd = rng.uniform(-0.3, 0.3, size=(2, c.cs)).astype(f32)
            q = (fwd[1] + rng.normal(0, 0.01, size=c.cs)).astype(f32)[None]
            s = _seq_s(q[0], variants(fwd))
            if s[4:].min() < s[:4].min():  # the nearest is a variant of row 1
                break
        gap = f32(s[:4].min() - s[4:].min())
        eps = [np.nextafter(gap, f32(0)), gap, np.nextafter(gap, f32(1))][c.arg + 1]
    elif c.kind == "ieee_sqrt":
        fwd, q, eps = _IEEE[0].view(f32), _IEEE[1].view(f32), np.array([_IEEE[2]], np.uint32).view(f32)[0]
    else:
        raise ValueError(c.kind)
    fwd, q = np.ascontiguousarray(fwd, f32), np.ascontiguousarray(q, f32)
    assert fwd.shape == (c.r, c.cs) and q.shape == (c.n, c.cs)
    fwd.setflags(write=False)
    q.setflags(write=False)
    return fwd, q, float(eps)


@functools.lru_cache(maxsize=None)
def want(case):
    import oracle_ffi

    fwd, q, eps = data(case)
    out = oracle_ffi.knnfit_assign(fwd, q, eps)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model(case, ftz=False):
    """(smallest tied index, tie count) per query"""
    fwd, q, eps = data(case)
    var = variants(fwd)
    best = np.zeros(len(q), np.int32)
    cnt = np.zeros(len(q), np.int64)
    with np.errstate(all="ignore"):
        for i in range(len(q)):
            s = _seq_s(q[i], var, ftz)
            d = np.abs(s - s.min())  # |s0 - sj|, one float32 subtraction either way round
            tied = np.flatnonzero(d <= f32(eps))
            best[i], cnt[i] = tied[0], len(tied)
    return best, cnt


def overflow(case):
    """queries whose tie set does not fit the bucket"""
    return int((model(case)[1] > BUCKET).sum())


# ---- the matrix --------------------------------------------------------------
EPS = 0.0026

CS_SWEEP = [Case("sweep", cs, 33, 257, EPS, 0, 1) for cs in range(1, 17)]
# every variant ties: 4R = 4, 8, 60, 64 fit the bucket, 68 does not
R_EDGES = [Case("sweep", cs, r, 40, 10.0, 0, 2) for cs in (8, 5) for r in (1, 2, 15, 16, 17)]
BUCKET_M = (63, 64, 65, 66)
BUCKET_WAYS = ("zero", "eps", "order")
# way "order": seeds at which the oracle's answer at 65 / 66 copies is not the smallest copy
# (test_knnfit_cases_host.py holds the condition; a seed that stops meeting it is replaced)
ORDER_SEED = 37
BUCKET_EDGES = {(m, way): Case("bucket", 8, m + 40, 12, 5e-4 if way == "eps" else 0.0, (m, way),
                               ORDER_SEED if way == "order" else 4)
                for m in BUCKET_M for way in BUCKET_WAYS}
TILE_CS = (8, 15, 16)
TILE_EDGES = {cs: [Case("tile", cs, r, 64, 1e-4, None, 5)
                   for r in (tile_rows(cs) - 1, tile_rows(cs), tile_rows(cs) + 1, 2 * tile_rows(cs) + 1)]
              for cs in TILE_CS}
# a tie set that straddles the tile edge: 64 + 1 overflows, 63 + 1 does not, so the count across tiles shows
TILE_TIES = {cs: [Case("tiletie", cs, tile_rows(cs) + 2, 12, 0.0, m, 5) for m in (64, 63)] for cs in TILE_CS}
N_EDGES = [Case("sweep", 8, 40, n, EPS, 0, 6) for n in (1, 255, 256, 257, 513)]
SCALES = [Case("sweep", 8, 33, 257, EPS, p, 1) for p in (-60, -70, 10)]
BIG_CAND = Case("bigcand", 8, 33, 257, EPS, None, 7)
BIG_QUERY = Case("bigquery", 8, 33, 257, EPS, None, 7)
# eps on the decision boundary: an inexact sqrt flips the choice
GAPS = {cs: [Case("gap", cs, 2, 1, 0.0, a, s) for s in range(16) for a in (-1, 0, 1)] for cs in (4, 8, 16)}
IEEE_SQRT = Case("ieee_sqrt", 8, 2, 1, 0.0, None, 0)

# several frames in one launch
MIXED = [Case("sweep", 8, 1, 1, 0.001, 0, 8), Case("sweep", 8, 17, 300, 10.0, 0, 8),
         Case("tile", 8, 2049, 64, 1e-4, None, 8), Case("sweep", 8, 16, 257, 9.0, 0, 8),
         Case("copies", 8, 600, 513, 0.0005, 70, 8)]
REPEAT = [MIXED[1], CS_SWEEP[7], Case("copies", 8, 100, 65, 0.0, 20, 9)] * 2


def all_cases():
    seen, out = set(), []
    groups = [CS_SWEEP, R_EDGES, list(BUCKET_EDGES.values()), [c for v in TILE_EDGES.values() for c in v],
              [c for v in TILE_TIES.values() for c in v], N_EDGES,
              SCALES, [BIG_CAND, BIG_QUERY, IEEE_SQRT], [c for v in GAPS.values() for c in v], MIXED, REPEAT]
    for c in (c for g in groups for c in g):
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def case_id(c):
    return f"{c.kind}-cs{c.cs}-r{c.r}-n{c.n}-{c.arg}-s{c.seed}"
