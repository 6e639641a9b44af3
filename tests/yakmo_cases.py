"""Inputs for the yakmo seeding kernel (gsc_yakmo.hip yakmo_seed2_kernel) and a
path model of what each input makes it do.

  gen(kind, n, d, seed)   deterministic datasets, one generator per data kind
  model(x, k)             oracle/yakmo_oracle.c restated in numpy float32
                          (vectorised over points; np.cumsum(dtype=float32)
                          is the sequential chain), with the statistics that
                          say which of the kernel's mechanisms an input
                          reaches, and the kernel's Elkan bookkeeping replayed
                          on the model's own distances
  oracle_seed_means(x, k) the oracle's centroids and labels, cached by case
  the case matrix         shared by test_yakmo_cases_host.py (the model equals
                          the oracle, every kind meets its condition) and
                          test_gpu_yakmo_matrix.py (the kernel equals the oracle)

Plain module: no fixtures, no GPU.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np

f32 = np.float32
FLT_MAX = f32(3.4028235e38)

# one frame: n points of d columns (the stage entry pads rows to the stride 8 / 16 / 32), k seeds
Case = namedtuple("Case", "kind n d k seed")


def step_points(d):
    """Points per pipeline step: 1024 at stride 8 / 16, 512 at 32."""
    return 512 if d > 16 else 1024


def gen(kind, n, d, seed):
    rng = np.random.default_rng([seed, n, d])
    g = lambda *s: rng.standard_normal(s).astype(f32)  # noqa: E731
    if kind == "gauss":
        return g(n, d) * f32(50.0)
    if kind == "integer":  # many equal distances and duplicate points
        return rng.integers(-3, 4, size=(n, d)).astype(f32)
    if kind == "integer_wide":  # totals beyond 2^24 with exact half-ulp ties
        return rng.integers(-24, 25, size=(n, d)).astype(f32)
    if kind == "silence":
        return np.zeros((n, d), f32)
    if kind == "signed_zero":
        x = np.zeros((n, d), f32)
        x[::3] = f32(-0.0)
        x[n - 50:] = rng.integers(-3, 4, size=(50, d)).astype(f32)
        return x
    if kind == "quiet_tail":
        x = np.zeros((n, d), f32)
        x[n - 3:] = g(3, d)
        return x
    if kind == "dup":
        return (g(5, d) * f32(50.0))[rng.integers(0, 5, size=n)]
    if kind == "offset":  # the expanded form |c|^2 + |x|^2 - 2 x.c is all rounding noise
        return f32(1000.0) + f32(0.01) * g(n, d)
    if kind == "clusters":
        return (f32(1000.0) * g(12, d))[rng.integers(0, 12, size=n)] + f32(0.5) * g(n, d)
    if kind == "lattice":  # seed distances tie exactly
        c = rng.integers(-4, 5, size=(12, d)).astype(f32) * f32(512.0)
        return c[rng.integers(0, 12, size=n)] + rng.integers(-1, 2, size=(n, d)).astype(f32)
    if kind == "cep":  # the encoder's scale: the cepstrum half is tiny
        x = g(n, d)
        x[:, d // 2:] *= f32(1e-5)
        return x
    if kind == "outliers":  # the prefix jumps across many binades at once
        x = g(n, d)
        x[rng.integers(0, n, size=max(1, n // 500))] *= f32(1e4)
        return x
    if kind == "overflow":  # finite norms, the total overflows
        x = g(n, d)
        x[rng.choice(n, 40, replace=False)] *= f32(1.5e18)
        return x
    if kind == "nan":
        x = g(n, d) * f32(50.0)
        x[int(rng.integers(0, n)), int(rng.integers(0, d))] = np.nan
        return x
    raise ValueError(kind)


def _lower_bound(cum, target):
    first, count = 0, len(cum)
    while count > 0:
        half = count >> 1
        mid = first + half
        if target > cum[mid]:
            first = mid + 1
            count -= half + 1
        else:
            count = half
    return first


def model(x, k, elkan=True):
    """Labels of the seeding assignment and the path statistics (a dict)."""
    x = np.ascontiguousarray(x, dtype=f32)
    n, d = x.shape
    assert 0 < k < n
    st = dict(nonpart=0, zero_total=0, neg_total=0, nonfinite_total=0, walk_steps=0, wraps=0, lb_n=0, ties=0,
              first_total=None, skipped=0, unsound=0, neg_d0=0)
    with np.errstate(all="ignore"):
        norm = np.zeros(n, f32)
        for j in range(d):
            norm = norm + x[:, j] * x[:, j]
        xmax = f32(np.max(np.where(np.isnan(norm), FLT_MAX, norm), initial=f32(0)))
        x2 = x + x
        d0 = np.zeros(n, f32)
        ids = np.zeros(n, np.int32)
        chosen = np.zeros(n, bool)
        seeds = np.zeros((k, d), f32)
        cum = None
        neg_any = np.zeros(n, bool)
        total = f32(0)
        cmax = f32(0)
        s = [123456789, 362436069, 521288629, 88675123]
        M = (1 << 64) - 1
        for i in range(k):
            t = (s[0] ^ (s[0] << 11)) & M
            s[0], s[1], s[2] = s[1], s[2], s[3]
            s[3] = (s[3] ^ (s[3] >> 19) ^ t ^ (t >> 8)) & M
            r = f32(np.float64(s[3]) * 5.42101086242752217e-20)
            if i == 0:
                idx = int(np.floor(r * f32(n)))
            else:
                target = r * total
                idx = _lower_bound(cum, target)
                below = target > cum
                st["nonpart"] += int(below[np.argmin(below):].any()) if not below.all() else 0
                st["lb_n"] += idx == n
                st["zero_total"] += bool(total == 0)
                st["neg_total"] += bool(total < 0)
                st["nonfinite_total"] += not np.isfinite(total)
            if idx < n and chosen[idx]:  # the collision walk, by its end point
                free = np.flatnonzero(~chosen)
                j = int(np.searchsorted(free, idx))
                if j < len(free):
                    st["walk_steps"] += int(free[j]) - idx
                    idx = int(free[j])
                else:
                    st["walk_steps"] += n - idx + int(free[0])
                    st["wraps"] += 1
                    idx = int(free[0])
            if idx >= n:
                idx = n - 1
            chosen[idx] = True
            c = x[idx].copy()
            seeds[i] = c
            cn = norm[idx]
            cmax = cn if i == 0 else np.fmax(cmax, cn)
            dist = (cn + norm) + f32(0)
            for j in range(d):
                dist = dist - x2[:, j] * c[j]
            better = np.ones(n, bool) if i == 0 else d0 > dist
            if elkan and i > 0:  # the kernel's skip decision, on the old d0 / ids
                s2 = np.zeros(i, f32)
                for j in range(d):
                    tt = seeds[:i, j] - c[j]
                    s2 = s2 + tt * tt
                sdlo = s2 * f32(0.99998474)
                e = (xmax + cmax) * f32(1.52587891e-05)
                need = ((np.fmax(d0, f32(0)) + e) * f32(4.0)) * f32(1.00000381)
                skip = sdlo[ids] >= need
                st["skipped"] += int(skip.sum())
                st["unsound"] += int((skip & better).sum())
            d0 = np.where(better, dist, d0)
            ids[better] = i
            if i < k - 1:
                cum = np.cumsum(d0, dtype=f32)
                total = cum[-1]
                neg_any |= d0 < 0
                if i == 0:
                    st["first_total"] = float(total)
                # tie points: the running total is at least 2^24 and d0 an odd multiple of its half-ulp
                prev = cum[:-1].astype(np.float64)
                ok = np.isfinite(prev) & (prev >= 16777216.0)
                if ok.any():
                    _, ex = np.frexp(prev[ok])
                    q = d0[1:][ok].astype(np.float64) / np.ldexp(1.0, ex - 25)
                    st["ties"] += int(((q == np.floor(q)) & (np.mod(q, 2.0) == 1.0)).sum())
    st["neg_d0"] = int(neg_any.sum())  # points whose d0 was negative in some pick's chain
    st["empty"] = k - len(np.unique(ids))
    st["skip_share"] = st["skipped"] / float(n * max(k - 1, 1))
    return ids, st


_ORACLE = {}


def oracle_seed_means(x, k, key=None):
    """(centroids, labels) of ora_yakmo_seed_means; key caches the result."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    import oracle_ffi

    x = np.ascontiguousarray(x, dtype=f32)
    n, d = x.shape
    c = np.zeros((k, d), f32)
    lab = np.zeros(n, np.int32)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    assert oracle_ffi.load().ora_yakmo_seed_means(n, d, x.ctypes.data_as(fp), k, c.ctypes.data_as(fp),
                                                  lab.ctypes.data_as(ip)) == 0
    c.setflags(write=False)
    lab.setflags(write=False)
    if key is not None:
        _ORACLE[key] = (c, lab)
    return c, lab


def data(case):
    return gen(case.kind, case.n, case.d, case.seed)


def want(case):
    return oracle_seed_means(data(case), case.k, key=case)


# ---- the matrix --------------------------------------------------------------
STRIDES = (8, 16, 32)


def n_sweep(d):
    s = step_points(d)
    return [3, 63, 64, 65, s - 1, s, s + 1, s + 517, s + 576, 2 * s + 1, 3 * s - 1, 3 * s, 3 * s + 1, 4 * s + 1,
            6 * s + 7]


N_SWEEP = {(d, kind): [Case(kind, n, d, min(n - 1, 48), 1) for n in n_sweep(d)]
           for d in STRIDES for kind in ("gauss", "integer")}
# the smallest colCount of each stride (rows zero-padded by the stage entry), at N = S + 1
SMALL_COLS = {d: Case("gauss", step_points(d) + 1, cols, 48, 2) for cols, d in ((2, 8), (10, 16), (18, 32))}

K_VALUES = [1, 2, 3, 63, 64, 65, 511, 512, 513, 1025, 4095, 4096]


def _k_cases(d, ks):
    return [Case("gauss", n, d, k, 3) for k in ks for n in (k + 1, max(2 * k, 600) + 3)]


K_SWEEP = {16: _k_cases(16, K_VALUES), 8: _k_cases(8, [1, 2, 513, 4096]), 32: _k_cases(32, [1, 2, 513, 4096])}
K_ALL_CHOSEN = [Case("integer", n, 16, n - 1, 4) for n in (65, 300, 1030)]

# kind -> (n, k) per stride; seeds chosen so that every kind meets its condition
# (test_yakmo_cases_host.py): a seed that stops meeting one is replaced, never the condition
KIND_SHAPES = {
    "silence": (130, 7), "signed_zero": (1500, 16), "quiet_tail": (200, 9), "dup": (1500, 40),
    "offset": (1500, 64), "clusters": (2500, 48), "lattice": (2500, 48), "cep": (3100, 64),
    "outliers": (2100, 32), "overflow": (1500, 16), "nan": (1500, 16),
}
KIND_SEEDS = {("quiet_tail", 8): 6, ("quiet_tail", 16): 6, ("quiet_tail", 32): 7, ("dup", 8): 6, ("dup", 32): 8}
KINDS = {d: [Case(kind, n, d, k, KIND_SEEDS.get((kind, d), 5)) for kind, (n, k) in KIND_SHAPES.items()]
         for d in STRIDES}
INTEGER_WIDE = Case("integer_wide", 3100, 16, 48, 5)
DUP_MAX_K = Case("dup", 4200, 8, 4096, 5)

BOUNDARY = [Case("integer", 262144, 8, 5, 6), Case("integer", 262145, 8, 5, 6), Case("gauss", 262144, 32, 5, 6),
            Case("gauss", 262145, 32, 5, 6)]

# several frames in one launch: (d, [cases])
_MIXED = [(65, 7), (1025, 33), (300, 299), (3073, 48), (64, 63)]
MIXED = (16, [Case("gauss", n, 16, k, 7) for n, k in _MIXED])
_BIG = Case("integer", 262145, 8, 4, 7)
_SMALL8 = [Case("gauss", n, 8, k, 7) for n, k in _MIXED[:3]]
MIXED_BIG_FIRST = (8, [_BIG] + _SMALL8)
MIXED_BIG_LAST = (8, _SMALL8 + [_BIG])
REPEAT = (16, [Case("gauss", 1025, 16, 33, 7), Case("integer", 300, 16, 299, 4), Case("gauss", 65, 16, 7, 7)] * 2)


def single_cases():
    """Every one-frame case of the matrix."""
    out = [c for v in N_SWEEP.values() for c in v] + list(SMALL_COLS.values())
    out += [c for v in K_SWEEP.values() for c in v] + K_ALL_CHOSEN
    out += [c for v in KINDS.values() for c in v] + [INTEGER_WIDE, DUP_MAX_K] + BOUNDARY
    return out


def all_cases():
    seen, out = set(), []
    for c in single_cases() + MIXED[1] + MIXED_BIG_FIRST[1] + MIXED_BIG_LAST[1] + REPEAT[1]:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def case_id(c):
    return f"{c.kind}-n{c.n}-d{c.d}-k{c.k}"
