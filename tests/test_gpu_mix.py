"""Gain-weighted sums of crops (``CropBinding.mix``) against the definition of
include/soundchunks.h: every source's int64 row comes from the oracle's PCM
through ``model_row`` of test_gpu_decode_resample.py (the definition of a crop,
resampled or not), and the formula ``clamp((sum gain * x + 16384) >> 15)`` is
applied in numpy int64.  Every comparison is exact.  ``out`` is pre-filled with
0x5555 (float32: 0x55555555) and ``written`` with -7, so an element the kernel
skipped shows.  Crafted streams as in test_gpu_crops_bound.py: 4500 samples,
ChunkSize 3, two frames around an empty one.

No decoded stream holds -32768 (a search over both bit depths, every
attenuation and dividers 1 to 63 found none: the synthesis never wraps to it),
so the inversion of -32768 runs on the rail-to-rail stream through the
resampler, whose clamp gives it; the test asserts that it is there.
"""
from __future__ import annotations

import numpy as np
import pytest

import gsc_writer as gw
import oracle_ffi  # noqa: F401  (Res decodes through it)
from golden.cases import HERE
from test_gpu_crops_bound import prefilled
from test_gpu_decode_resample import Res, craft, model_row

pytestmark = pytest.mark.gpu

UNITY = 32768
FMTS = [("int16", "TC"), ("float32", "CT")]


@pytest.fixture(scope="module")
def sc():
    import soundchunks_amd

    return soundchunks_amd


@pytest.fixture(scope="module")
def crafted(sc):
    """Streams of 4500 samples per (rate, channels, variant), made once."""
    made = {}

    def get(rate, ch, variant=0):
        if (rate, ch, variant) not in made:
            made[rate, ch, variant] = Res(sc, craft(100 + rate % 97 + ch + 50 * variant, ch, rate))
        return made[rate, ch, variant]

    return get


@pytest.fixture(scope="module")
def rails(sc):
    """test_saturation's stream of test_gpu_decode_resample.py: jumps between the rails at full volume."""
    rng = np.random.default_rng(7)
    syms = [(int(rng.integers(0, 2)), int(rng.integers(0, 2)), 0 if i == 0 else None, int(rng.integers(0, 2)))
            for i in range(400)]
    r = Res(sc, gw.frame(syms, ch=1, count=2, cs=3, rate=32000, att=[0, 0], codes=[[255, 0, 255], [0, 255, 0]]))
    assert r.ref.min() < -32000 and r.ref.max() > 32000
    return r


_rows = {}


def source_row(sc, r, begin, count, rate, channels):
    """model_row, once per crop: the references are shared and never written."""
    key = (id(r), begin, count, rate, channels)
    if key not in _rows:
        y, w, _ = model_row(sc, r, begin, count, rate, channels)
        y = np.ascontiguousarray(y, np.int64)
        y.setflags(write=False)
        _rows[key] = (y, w)
    return _rows[key]


def source_bad(rs, s, begin, count, gain, length):
    return (not 0 <= s < len(rs) or begin < 0 or begin > len(rs[s].ref) or count < 0 or count > length or
            abs(gain) > 1 << 20)


def expected(sc, rs, sources, length, dtype, layout, rate, channels):
    """(rows as the call returns them, written, the int64 sums before the clamp) by the definition."""
    import torch

    co = rs[0].ch if channels is None else channels
    R = len(sources)
    raw = np.zeros((R, length, co), np.int64)
    written = []
    for i, row in enumerate(sources):
        if any(source_bad(rs, *src, length) for src in row):
            written.append(-1)
            continue
        longest = 0
        for s, begin, count, gain in row:
            if count == 0:
                continue
            y, w = source_row(sc, rs[s], begin, count, rate, channels)
            raw[i, :w] += gain * y
            longest = max(longest, w)
        written.append(longest)
    raw = (raw + 16384) >> 15
    want = np.clip(raw, -32768, 32767).astype(np.int16)
    if dtype == torch.float32:
        want = want.astype(np.float32) / 32768
    return (want.transpose(0, 2, 1) if layout == "CT" else want), written, raw


def run(b, rs, sources, length, dtype, layout):
    import torch

    device = torch.device("cuda", rs[0].st.device)
    R, co = len(sources), b.channels
    out = prefilled((R, length, co) if layout == "TC" else (R, co, length), dtype, device)
    written = torch.full((R,), -7, dtype=torch.int64, device=device)
    t = torch.tensor(sources, dtype=torch.int64, device=device).reshape(R, -1, 4)
    x, n = b.mix(t, length, dtype=dtype, layout=layout, out=out, written=written)
    assert x is out and n is written
    stats = b.last_call()
    assert (stats["launches"], stats["allocations"], stats["copies"], stats["synchronisations"]) == (1, 0, 0, 0)
    return x, n


def check(sc, b, rs, sources, length, dtype=None, layout="TC", rate=None, channels=None):
    import torch

    dtype = torch.int16 if dtype is None else dtype
    want, lens, raw = expected(sc, rs, sources, length, dtype, layout, rate, channels)
    x, n = run(b, rs, sources, length, dtype, layout)
    got = x.cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (rate, channels, layout, length, len(bad), bad[:4].tolist(),
                           [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]])
    assert n.tolist() == lens, (n.tolist(), lens)
    return x, n, raw


def lengths_of(b):
    tile = b.mix_tile()
    return [1, tile - 1, tile, tile + 1, 2 * tile + 7]


def random_sources(rng, rs, R, K, length, gain_span=1 << 16):
    """Sources that start in either frame, straddle the empty one (frame 0 holds 2100 samples), end past the
    stream's end, and fall at every offset inside a chunk."""
    n = len(rs[0].ref)
    begins = [0, 7, 31, 32, 1000, 2100 - 20, 2099, 2100, 3000, n - 50, n - 1, n]
    rows = []
    for _ in range(R):
        row = []
        for _ in range(K):
            count = int(rng.choice([length, length, max(1, length // 2), max(1, length - 3), 1]))
            row.append((int(rng.integers(0, len(rs))), int(rng.choice(begins)), count,
                        int(rng.integers(-gain_span, gain_span + 1))))
        rows.append(row)
    return rows


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("rate,ch", [(None, 1), (None, 2), (44100, 2)])
def test_one_source_at_unity_is_decode_crops(sc, crafted, rate, ch, fmt):
    import torch

    r = crafted(32000, ch)
    n = len(r.ref)
    b = sc.Decoder.bind([r.st], rate=rate)
    dtype, layout = getattr(torch, fmt[0]), fmt[1]
    device = torch.device("cuda", r.st.device)
    assert b.mix_tile() == (sc.Decoder.resample_tile() if rate else 4096 // ch)
    for length in lengths_of(b):
        crops = [(0, 0, length), (0, 2090, min(length, 40)), (0, n - 50, length), (0, n, min(length, 3)), (0, 5, 0),
                 (0, 100, length), (0, 1, max(1, length - 1))]
        t = torch.tensor(crops, dtype=torch.int64, device=device)
        xd, nd = b.decode_crops(t, length, dtype=dtype, layout=layout)
        sources = [[(s, bg, c, UNITY)] for s, bg, c in crops]
        x, w = run(b, [r], sources, length, dtype, layout)
        assert torch.equal(x, xd) and torch.equal(w, nd), length
    b.close()


PAIRS = [  # streams as (rate, channels), the binding's rate and channels
    ([(32000, 1)], None, None), ([(32000, 2)], None, None),
    ([(32000, 1)], 44100, None), ([(32000, 2)], 44100, None), ([(48000, 2), (32000, 2)], 44100, None),
    ([(32000, 1)], 8000, None), ([(32000, 1), (32000, 2)], None, 2),
]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("specs,rate,channels", PAIRS)
def test_parity_with_the_model(sc, crafted, specs, rate, channels, fmt):
    import torch

    rs = [crafted(fi, ch) for fi, ch in specs] + [crafted(specs[0][0], specs[0][1], 1)]
    b = sc.Decoder.bind([r.st for r in rs], rate=rate, channels=channels)
    rng = np.random.default_rng(len(specs) + (rate or 0))
    dtype, layout = getattr(torch, fmt[0]), fmt[1]
    lengths = lengths_of(b)
    for length, K in zip(lengths + lengths[-1:] * 3, [2, 3, 5, 1, 2, 1, 3, 5]):
        sources = random_sources(rng, rs, 6, K, length)
        check(sc, b, rs, sources, length, dtype, layout, rate, channels)
    b.close()


@pytest.mark.parametrize("rate", [None, 44100])
def test_rounding_and_sign(sc, crafted, rails, rate):
    rs = [crafted(32000, 1), rails]
    b = sc.Decoder.bind([r.st for r in rs], rate=rate)
    length = b.mix_tile() + 1
    # the same crop at +g and -g cancels exactly; one half of odd samples rounds half up; full inversion
    sources = [[(0, 10, length, 12345), (0, 10, length, -12345)],
               [(0, 2090, length, 1 << 20), (0, 2090, length, -(1 << 20))],
               [(0, 0, length, 16384), (0, 5, 0, 0)],
               [(1, 0, length, -UNITY), (0, 5, 0, 0)],
               [(0, 3, length, -UNITY), (0, 5, 0, 0)]]
    x, n, _ = check(sc, b, rs, sources, length, rate=rate)
    assert not x[:2].any().item() and n[0].item() == length and n[1].item() > 0
    y, w = source_row(sc, rs[0], 0, length, rate, None)
    odd = y[(y & 1) == 1]
    assert (odd > 0).any() and (odd < 0).any()  # odd samples of both signs meet the half-way round
    if rate:
        y, _ = source_row(sc, rails, 0, length, rate, None)
        assert (y == -32768).any()  # the clamp of the resampler: -(-32768) must clamp again
        row = x[3, :, 0].cpu().numpy()
        assert (row[:len(y)][y[:, 0] == -32768] == 32767).all()
    b.close()


@pytest.mark.parametrize("rate", [None, 44100])
def test_saturation(sc, rails, rate):
    import torch

    b = sc.Decoder.bind([rails.st], rate=rate)
    length = 1500
    crop = (0, 0, length)
    sources = [[crop + (UNITY,), crop + (UNITY,), (0, 0, 0, 0)],
               [crop + (1 << 20,)] * 3,
               [crop + (-(1 << 20),)] * 3,
               [crop + (UNITY,), (0, 333, 700, UNITY), (0, 7, 0, 0)]]
    _, _, raw = check(sc, b, [rails], sources, length, rate=rate)
    for i in range(3):
        assert (raw[i] > 32767).any() and (raw[i] < -32768).any()  # the model clamps both ways: not vacuous
    check(sc, b, [rails], sources, length, torch.float32, "CT", rate=rate)
    b.close()


@pytest.mark.parametrize("rate", [None, 44100])
def test_empty_slots_and_written(sc, crafted, rate):
    rs = [crafted(32000, 2), crafted(32000, 2, 1)]
    n = len(rs[0].ref)
    b = sc.Decoder.bind([r.st for r in rs], rate=rate)
    length = 2 * b.mix_tile() + 7
    e = (1, 9, 0, 777)  # an empty slot: it adds nothing whatever its gain
    sources = [[(0, 0, length, 20000), (1, 40, 300, -9000), (0, 2000, length - 5, 4000)],  # no empty slot
               [(0, 0, 100, 20000), e, (1, 40, 300, -9000)],                                # one
               [e, e, (0, 50, 70, UNITY)],                                                   # K - 1
               [e, e, e],                                                                    # all: zero, written 0
               [(0, n - 60, length, UNITY), (1, 10, 20, UNITY), e],     # the longest source is clipped at the end
               [(0, n, length, UNITY), (1, n - 1, length, UNITY), e]]   # one behind the end, one on the last sample
    x, w, _ = check(sc, b, rs, sources, length, rate=rate)
    lens = w.tolist()
    assert lens[0] == length and lens[3] == 0 and not x[3].any().item()
    assert 20 < lens[4] < length and not x[4, lens[4]:].any().item() and x[4, :lens[4]].any().item()
    if rate is None:
        assert lens[1:3] == [300, 70] and lens[4] == 60 and lens[5] == 1
    b.close()


@pytest.mark.parametrize("rate", [None, 44100])
def test_bad_rows(sc, crafted, rate):
    """Each kind of bad source in the first, a middle and the last slot of one of five rows in turn: that row is
    zero with written -1, the other four are what they are without it."""
    import torch

    rs = [crafted(32000, 2), crafted(32000, 2, 1)]
    n, length, K = len(rs[0].ref), 300, 3
    b = sc.Decoder.bind([r.st for r in rs], rate=rate)
    rng = np.random.default_rng(3)
    base = random_sources(rng, rs, 5, K, length)
    x0, w0, _ = check(sc, b, rs, base, length, rate=rate)
    kinds = [(-1, 0, 5, UNITY), (len(rs), 0, 5, UNITY), (0, -1, 5, UNITY), (1, n + 1, 5, UNITY),
             (0, 5, -1, UNITY), (1, 5, length + 1, UNITY), (0, 5, 5, (1 << 20) + 1), (1, 5, 5, -(1 << 20) - 1)]
    turn = 0
    for kind in kinds:
        for slot in (0, 1, K - 1):
            row = turn % 5
            turn += 1
            sources = [list(r) for r in base]
            sources[row][slot] = kind
            x, w, _ = check(sc, b, rs, sources, length, rate=rate)
            keep = torch.arange(5, device=x.device) != row
            assert not x[row].any().item() and w[row].item() == -1
            assert torch.equal(x[keep], x0[keep]) and torch.equal(w[keep], w0[keep])
    # a bad value in an empty slot, and values far outside int32
    for kind in [(0, 5, 0, (1 << 20) + 1), (7, 0, 0, 0), (1 << 40, 0, 5, 1), (0, 1 << 62, 5, 1), (0, 5, 5, 1 << 62),
                 (0, 5, 5, -(1 << 63))]:
        sources = [list(r) for r in base]
        sources[2][1] = kind
        x, w, _ = check(sc, b, rs, sources, length, torch.float32, "CT", rate=rate)
        assert not x[2].any().item() and w[2].item() == -1
    b.close()


def test_contract_and_degenerate_shapes(sc, crafted):
    import torch

    r = crafted(32000, 2)
    device = torch.device("cuda", r.st.device)
    for rate in (None, 44100):
        b = sc.Decoder.bind([r.st], rate=rate)
        t = torch.tensor([[(0, 0, 8, UNITY), (0, 9, 8, 5)]] * 3, dtype=torch.int64, device=device)
        b.mix(t, 8)
        stats = b.last_call()
        assert (stats["launches"], stats["allocations"], stats["copies"], stats["synchronisations"]) == (1, 0, 0, 0)
        w = torch.full((0,), -7, dtype=torch.int64, device=device)
        x, n = b.mix(torch.empty((0, 2, 4), dtype=torch.int64, device=device), 64, written=w)
        assert tuple(x.shape) == (0, 64, 2) and n is w and b.last_call()["launches"] == 0
        w = torch.full((3,), -7, dtype=torch.int64, device=device)
        t0 = torch.tensor([[(0, 0, 0, UNITY), (0, 9, 0, 5)]] * 3, dtype=torch.int64, device=device)
        x, n = b.mix(t0, 0, layout="CT", written=w)
        assert tuple(x.shape) == (3, 2, 0) and b.last_call()["launches"] == 0
        assert n.tolist() == [-7, -7, -7]  # nothing launched: written is as it was
        b.close()


def test_refusals(sc, crafted):
    import torch
    from soundchunks_amd import _lib

    r = crafted(32000, 2)
    device = torch.device("cuda", r.st.device)
    b = sc.Decoder.bind([r.st])
    t = torch.tensor([[(0, 0, 10, UNITY), (0, 5, 10, 100)]], dtype=torch.int64, device=device)
    out = prefilled((1, 64, 2), torch.int16, device)
    written = torch.full((1,), -7, dtype=torch.int64, device=device)
    wide = torch.zeros((1, 257, 4), dtype=torch.int64, device=device)
    calls = [dict(sources=torch.empty((1, 0, 4), dtype=torch.int64, device=device)), dict(sources=wide),
             dict(sources=t.to(torch.int32)), dict(sources=wide[:, ::2]), dict(sources=t.cpu()),
             dict(sources=t[:, :, :3]), dict(sources=t.reshape(2, 4)), dict(sources=[[(0.5, 0, 1, 1)]]),
             dict(sources=t, out=out.cpu()), dict(sources=t, out=out[:, :32]),
             dict(sources=t, out=out.view(torch.float16)), dict(sources=t, dtype=torch.float16),
             dict(sources=t, layout="TCB"), dict(sources=t, length=-1),
             dict(sources=t, written=torch.zeros(1, dtype=torch.int32, device=device))]
    for kw in calls:
        kw.setdefault("out", out)
        kw.setdefault("written", written)
        with pytest.raises((sc.GscError, ValueError)) as e:
            b.mix(kw.pop("sources"), kw.pop("length", 64), **kw)
        assert str(e.value).strip(), kw
    torch.cuda.synchronize()
    assert (out == 0x5555).all().item() and written.tolist() == [-7]  # none of them launched
    # the C entry point refuses the source counts too, before any launch
    lib = sc.load()
    for nsrc in (0, 257, -1):
        assert lib.gsc_crop_binding_mix(b._h, wide.data_ptr(), 1, nsrc, _lib.PCM_INT16, _lib.LAYOUT_TC, 64,
                                        out.data_ptr(), written.data_ptr(), None) != 0
        assert b.last_call()["launches"] == 0 and "sources" in lib.gsc_last_error().decode()
    # a host list is uploaded by the wrapper, and a correct call still works
    x, w = b.mix([[(0, 0, 10, UNITY), (0, 5, 0, 100)]], 64, out=out, written=written)
    assert w.tolist() == [10] and np.array_equal(x[0, :10].cpu().numpy(), r.ref[:10]) and not x[0, 10:].any().item()
    b.close()
    with pytest.raises(sc.GscError, match="closed"):
        b.mix(t, 64)


def test_closed_streams(sc):
    import torch

    gscs = [craft(300 + i, 2, 32000, rows=(100, 120)) for i in range(3)]
    ss = sc.Decoder.open_many(gscs[:2])
    single = sc.Decoder.open(gscs[2])
    device = torch.device("cuda", single.device)
    t = torch.tensor([[(0, 0, 10, UNITY), (2, 5, 10, UNITY)]], dtype=torch.int64, device=device)
    b1, b2 = sc.Decoder.bind(ss.streams + [single]), ss.bind()
    b1.mix(t, 16)
    b2.mix(t[:, :1], 16)
    single.close()
    with pytest.raises(sc.GscError, match="closed"):
        b1.mix(t, 16)
    b2.mix(t[:, :1], 16)  # the set is still open
    ss.close()
    with pytest.raises(sc.GscError, match="closed"):
        b2.mix(t[:, :1], 16)
    b1.close()
    b2.close()


@pytest.mark.parametrize("names,rate,channels", [
    (["square_empty_frame0_cs4", "syn2s_cs7_mono_cbd12"], None, None),
    (["syn13s_48k_cs4_cpf256_fl13000", "hihat_cs8_cpf256"], 44100, 2)])
def test_goldens(sc, names, rate, channels):
    rs = [Res(sc, (HERE / f"{name}.gsc").read_bytes()) for name in names]
    b = sc.Decoder.bind([r.st for r in rs], rate=rate, channels=channels)
    rng = np.random.default_rng(len(names[0]))
    length = 2 * b.mix_tile() + 7 if rate else 5000  # more than one tile either way
    sources = []
    for _ in range(6):
        row = []
        for _ in range(3):
            s = int(rng.integers(0, len(rs)))
            row.append((s, int(rng.integers(0, len(rs[s].ref) + 1)), int(rng.integers(1, length + 1)),
                        int(rng.integers(-(1 << 16), (1 << 16) + 1))))
        sources.append(row)
    sources[0] = [(0, 1000, length, UNITY), (1, 2000, length, 8192), (0, 0, 0, 0)]  # 1.0 and 0.25
    check(sc, b, rs, sources, length, rate=rate, channels=channels)
    b.close()
    for r in rs:
        r.st.close()


def test_stream_order(sc, crafted):
    """A mix enqueued on a side stream right after a torch op that writes its sources there is correct after
    that stream alone is synchronised."""
    import torch

    r = crafted(32000, 2)
    n, length = len(r.ref), 600
    device = torch.device("cuda", r.st.device)
    lists = [[[(0, 0, 600, UNITY), (0, 3000, 600, -8000)], [(0, n - 100, 600, 70000), (0, 7, 0, 1)]],
             [[(0, 2000, 100, 5), (0, 7, 600, -UNITY)], [(0, n, 3, UNITY), (0, 2090, 30, 16384)]]]
    b = sc.Decoder.bind([r.st])
    src = [torch.tensor(c, dtype=torch.int64, device=device) for c in lists]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    t = torch.zeros((2, 2, 4), dtype=torch.int64, device=device)
    got = []
    with torch.cuda.stream(side):
        for s in src:
            t.copy_(s)  # written on the side stream, read by the kernel enqueued behind it
            got.append(b.mix(t, length, out=prefilled((2, length, 2), torch.int16, device)))
    side.synchronize()
    for (x, w), c in zip(got, lists):
        want, lens, _ = expected(sc, [r], c, length, torch.int16, "TC", None, None)
        assert np.array_equal(x.cpu().numpy(), want) and w.tolist() == lens
    b.close()
