"""Crops at a common sample rate and channel count
(``Decoder.decode_crops(..., rate=, channels=)``) against the integer
definition of include/soundchunks.h, applied in numpy int64 to the oracle's
PCM of the same bytes (``oracle_ffi.decode``) with the library's exported table
(``Decoder.resample_table``, itself checked in test_resample_table.py).  Every
comparison is exact.  Crafted streams as in test_gpu_decode_crops.py:
StreamVersion 1, ChunkSize 3, more than two checkpoint segments of symbols per
frame, random reverse flags, an empty frame between the two that hold samples.
"""
from __future__ import annotations

from math import gcd

import numpy as np
import pytest

import gsc_writer as gw
import oracle_ffi
from golden.cases import HERE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    import soundchunks_amd

    return soundchunks_amd


def craft(seed, ch, rate, rows=(700, 800), cs=3, count=90):
    """Two frames of rows[0] and rows[1] symbol rows around an empty one: 3 * sum(rows) samples."""
    rng = np.random.default_rng(seed)
    e = gw.random_frame(rng, 0, ch=ch, count=5, cs=cs, rate=rate)
    return (gw.random_frame(rng, ch * rows[0], ch=ch, count=count, cs=cs, rate=rate) + e +
            gw.random_frame(rng, ch * rows[1], ch=ch, count=count, cs=cs, rate=rate, policy="always"))


class Res:
    """A stream (resident on its own, or a member of a set) beside the oracle's PCM of the same bytes."""

    def __init__(self, sc, gsc, st=None):
        want, ch, rate = oracle_ffi.decode(gsc)
        self.ref = want.reshape(-1, ch)
        self.rate, self.ch = rate, ch
        self.st = sc.Decoder.open(gsc) if st is None else st
        assert (self.st.channels, self.st.sample_rate, self.st.samples_per_channel) == (ch, rate, len(self.ref))


def model_row(sc, r, begin, count, rate, channels):
    """(int64 [written, channels or the stream's], written) of one crop, by the definition."""
    n_s, fo = len(r.ref), r.rate if rate is None else rate
    if fo == r.rate:
        w = min(count, n_s - begin)
        y = r.ref[begin:begin + w].astype(np.int64)
        sat = 0
    else:
        g = gcd(r.rate, fo)
        L, M = fo // g, r.rate // g
        table = sc.Decoder.resample_table(r.rate, fo).astype(np.int64)
        assert table.shape[0] == L
        T = table.shape[1] // 2
        w = min(count, -((-(n_s - begin) * L) // M))
        n = np.arange(w, dtype=np.int64)
        pos = begin * L + n * M
        i0, ph = pos // L, pos % L
        xp = np.pad(r.ref.astype(np.int64), ((T, T + 1), (0, 0)))  # sample s at xp[s + T]; zero outside the stream
        idx = i0[:, None] + np.arange(-T + 1, T + 1, dtype=np.int64)[None, :] + T
        acc = np.einsum("wt,wtc->wc", table[ph], xp[idx])
        raw = (acc + (1 << 23)) >> 24
        y = np.clip(raw, -32768, 32767)
        sat = int((raw != y).sum())
    cs = r.ch
    co = cs if channels is None else channels
    if co == cs:
        pass
    elif cs == 1:
        y = np.repeat(y, co, axis=1)
    else:
        assert co == 1
        y = (2 * y.sum(axis=1, keepdims=True) + cs) // (2 * cs)  # floor
    return y, w, sat


def expected(sc, rs, crops, length, dtype, layout, rate, channels):
    import torch

    co = rs[0].ch if channels is None else channels
    want = np.zeros((len(crops), length, co), np.int16)
    lens, sat = [], 0
    for i, (s, b, c) in enumerate(crops):
        y, w, k = model_row(sc, rs[s], b, c, rate, channels)
        want[i, :w] = y
        lens.append(w)
        sat += k
    if dtype == torch.float32:
        want = want.astype(np.float32) / 32768
    return (want.transpose(0, 2, 1) if layout == "CT" else want), lens, sat


def check(sc, rs, crops, length, dtype=None, layout="TC", rate=None, channels=None, out=None):
    import torch

    dtype = torch.int16 if dtype is None else dtype
    x, n = sc.Decoder.decode_crops([r.st for r in rs], crops, length=length, dtype=dtype, layout=layout, out=out,
                                   rate=rate, channels=channels)
    want, lens, sat = expected(sc, rs, crops, length, dtype, layout, rate, channels)
    assert x.is_cuda and x.dtype == dtype and tuple(x.shape) == want.shape and x.is_contiguous()
    assert n == lens, (n, lens)
    got = x.cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (rate, channels, layout, len(bad), bad[:4].tolist(),
                           [(got[tuple(b)], want[tuple(b)]) for b in bad[:4]])
    return x, sat


@pytest.fixture(scope="module")
def crafted(sc):
    """Mono and stereo streams of 4500 samples at each source rate of the pairs below."""
    made = {}

    def get(rate, ch):
        if (rate, ch) not in made:
            made[rate, ch] = Res(sc, craft(100 + rate % 97 + ch, ch, rate))
        return made[rate, ch]

    return get


def edge_crops(sc, n, fi, fo):
    tile = sc.Decoder.resample_tile()
    many = 2 * tile + 7
    need = -(-many * fi // fo) + 2  # source samples `many` outputs read forward
    assert need + 100 < n
    crops = [(0, 0, 40),                      # the filter reads before sample 0: zeros
             (0, n - 50, many), (0, n - 1, 5), (0, n, 9),   # ending past the end, at its last sample, behind it
             (0, 2100 - 20, 60),              # across the frame boundary and the empty frame (frame 0: 2100 samples)
             (0, 2100, 33), (0, 2099, 1),
             (0, 30, 25), (0, 31, 25), (0, 32, 25),  # every offset inside a chunk
             (0, 500, 0), (0, 500, 1),
             (0, 100, many),                  # more than two tiles, unclipped
             (0, n - need, many)]             # ... and ending at the stream's end
    # a crop that ends exactly at the end: the last output's position is the last below n
    g = gcd(fi, fo)
    L, M = fo // g, fi // g
    exact = -((-(n - 1000) * L) // M)
    if exact <= many:
        crops.append((0, 1000, exact))
    return crops, many


@pytest.mark.parametrize("fmt", [("int16", "TC"), ("float32", "CT")])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("fi,fo", [(32000, 44100), (48000, 44100), (26390, 48000), (32000, 8000)])
def test_up_and_down(sc, crafted, fi, fo, ch, fmt):
    import torch

    r = crafted(fi, ch)
    crops, length = edge_crops(sc, len(r.ref), fi, fo)
    x, _ = check(sc, [r], crops, length, getattr(torch, fmt[0]), fmt[1], rate=fo)
    # rows past their written length are zero, and a crop behind the end is all zero
    assert not x[3].any()


def test_saturation(sc):
    """Two chunks of alternating extreme codes at full volume, negated at random:
    jumps between the rails, so the filter overshoots and the output clamps."""
    import torch

    rng = np.random.default_rng(7)
    syms = [(int(rng.integers(0, 2)), int(rng.integers(0, 2)), 0 if i == 0 else None, int(rng.integers(0, 2)))
            for i in range(400)]
    r = Res(sc, gw.frame(syms, ch=1, count=2, cs=3, rate=32000, att=[0, 0], codes=[[255, 0, 255], [0, 255, 0]]))
    assert r.ref.min() < -32000 and r.ref.max() > 32000
    crops = [(0, 0, 1500), (0, 333, 700)]
    for rate in (44100, 8000):
        _, sat = check(sc, [r], crops, 1500, rate=rate)
        if rate == 44100:
            assert sat > 0  # the model itself clamps: the case is not vacuous
    check(sc, [r], crops, 1500, torch.float32, "CT", rate=44100)


def test_identity(sc, crafted):
    """rate = the stream's own and channels = its own: the call without the keywords."""
    import torch

    for r in (crafted(32000, 1), crafted(48000, 2)):
        n = len(r.ref)
        crops = [(0, 0, 40), (0, n - 50, 100), (0, 2090, 30), (0, 31, 1100), (0, n, 3), (0, 7, 0)]
        for dtype, layout in ((torch.int16, "TC"), (torch.float32, "CT")):
            x, _ = check(sc, [r], crops, 1100, dtype, layout, rate=r.rate, channels=r.ch)
            x1 = sc.Decoder.decode_crops([r.st], crops, 1100, dtype=dtype, layout=layout, rate=r.rate)[0]
            x2 = sc.Decoder.decode_crops([r.st], crops, 1100, dtype=dtype, layout=layout, channels=r.ch)[0]
            assert torch.equal(x, x1) and torch.equal(x, x2)
            y, m = sc.Decoder.decode_crops([r.st], crops, 1100, dtype=dtype, layout=layout)
            assert torch.equal(x, y)
            assert m == [min(c, n - b) for _, b, c in crops]


def test_channels(sc, crafted):
    import torch

    mono = crafted(32000, 1)
    n = len(mono.ref)
    crops = [(0, 0, 600), (0, n - 100, 600), (0, 2095, 10)]
    for co in (2, 4):
        check(sc, [mono], crops, 600, channels=co)                       # native rate
        check(sc, [mono], crops, 600, torch.float32, "CT", rate=44100, channels=co)
    # stereo to mono: small samples, so that odd and negative sums occur
    rng = np.random.default_rng(0)
    count = 40
    quiet = Res(sc, gw.frame(gw.random_symbols(rng, 2 * 300, count), ch=2, count=count, cs=3, rate=32000,
                             att=rng.integers(10, 16, count), codes=rng.integers(118, 139, (count, 3))))
    sums = quiet.ref.astype(np.int64).sum(axis=1)
    assert (sums == -1).any() and (sums == 1).any() and (sums < -1).any() and (sums % 2 != 0).any()
    x, _ = check(sc, [quiet], [(0, 0, 900), (0, 450, 100)], 900, channels=1)
    got = x[0, :, 0].cpu().numpy()
    assert (got[sums == -1] == 0).all() and (got[sums == 1] == 1).all()  # -1/2 and 1/2 round up
    check(sc, [quiet], [(0, 0, 900), (0, 450, 100)], 1300, torch.float32, "CT", rate=44100, channels=1)
    stereo = crafted(48000, 2)
    check(sc, [stereo], [(0, 0, 700), (0, 4000, 700)], 700, rate=44100, channels=1)
    # 2 -> 3 is refused, the stream named, and nothing is written
    out = torch.full((1, 64, 3), 7, dtype=torch.int16, device=x.device)
    with pytest.raises(sc.GscError, match=r"stream 1 has 2 channels.*3"):
        sc.Decoder.decode_crops([mono.st, stereo.st], [(0, 0, 10)], 64, out=out, rate=44100, channels=3)
    torch.cuda.synchronize()
    assert (out == 7).all().item()
    with pytest.raises(sc.GscError, match="channels"):  # without channels= the streams must agree, as before
        sc.Decoder.decode_crops([mono.st, stereo.st], [(0, 0, 10)], 64, rate=44100)
    for bad in (dict(rate=0), dict(rate=-8000), dict(channels=0), dict(rate=1000)):  # 32000 -> 1000: over 512 taps
        with pytest.raises(sc.GscError) as e:
            sc.Decoder.decode_crops([mono.st], [(0, 0, 10)], 64, **bad)
        if bad.get("rate") == 1000:
            assert "32000" in str(e.value) and "1000" in str(e.value)


def test_mixed_batch(sc):
    """A set of four streams that differ in rate and channel count plus one
    opened on its own, one call to 44100 Hz stereo, crops in shuffled order."""
    import torch

    specs = [(26390, 1), (32000, 1), (44100, 2), (48000, 2)]
    gscs = [craft(200 + i, ch, rate, rows=(300, 350)) for i, (rate, ch) in enumerate(specs)]
    ss = sc.Decoder.open_many(gscs)
    rs = [Res(sc, g, st=ss[i]) for i, g in enumerate(gscs)]
    rs.append(Res(sc, craft(210, 1, 48000, rows=(300, 350))))
    n = len(rs[0].ref)
    assert n == 1950
    crops = []
    for s in range(len(rs)):
        crops += [(s, 0, 1200), (s, n - 300, 1200), (s, 890, 40), (s, 3 * s + 1, 1), (s, n, 4)]
    rng = np.random.default_rng(5)
    crops = [crops[i] for i in rng.permutation(len(crops))]
    for dtype in (torch.int16, torch.float32):
        for layout in ("TC", "CT"):
            x, _ = check(sc, rs, crops, 1200, dtype, layout, rate=44100, channels=2)
            out = torch.full_like(x, 7)
            y, _ = check(sc, rs, crops, 1200, dtype, layout, rate=44100, channels=2, out=out)
            assert y is out and torch.equal(x, out)
    # the set's own method counts its members
    x, m = ss.decode_crops([(3, 5, 100), (0, 5, 100)], 100, rate=44100, channels=2)
    want, lens, _ = expected(sc, rs, [(3, 5, 100), (0, 5, 100)], 100, torch.int16, "TC", 44100, 2)
    assert m == lens and np.array_equal(x.cpu().numpy(), want)
    wrong = torch.zeros((len(crops), 1200, 1), dtype=torch.int16, device=x.device)
    with pytest.raises(sc.GscError, match="out must be"):
        sc.Decoder.decode_crops([r.st for r in rs], crops, 1200, out=wrong, rate=44100, channels=2)
    rs[-1].st.close()
    ss.close()


@pytest.mark.parametrize("name,rate,channels", [("syn8s_48k_cs8_cpf4096", 44100, None), ("hihat_cs8_cpf256", 48000, 2)])
def test_goldens(sc, name, rate, channels):
    r = Res(sc, (HERE / f"{name}.gsc").read_bytes())
    n = len(r.ref)
    assert r.rate != rate
    back = 4410 * r.rate // rate  # source samples of 4410 outputs
    crops = [(0, 0, 4410), (0, n // 2, 4410), (0, n // 3 + 1, 4410), (0, n - back, 4410), (0, n - back // 2, 4410)]
    for fs in r.st.index.first_sample[1:-1][:2]:
        crops.append((0, max(int(fs) - back // 2, 0), 4410))
    check(sc, [r], crops, 4410, rate=rate, channels=channels)
    r.st.close()


def test_stream_order(sc, crafted):
    """On a stream of its own, after prepare_resample: correct after synchronising that stream alone."""
    import torch

    r = crafted(32000, 2)
    crops = [(0, 0, 1000), (0, 3000, 1000), (0, 2000, 700)]
    want, lens, _ = expected(sc, [r], crops, 1000, torch.float32, "CT", 22050, None)
    sc.Decoder.prepare_resample(32000, 22050)
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(s):
        x, n = sc.Decoder.decode_crops([r.st], crops, 1000, dtype=torch.float32, layout="CT", rate=22050)
        y = x * 2 + 1
    s.synchronize()
    assert n == lens
    assert np.array_equal(y.cpu().numpy(), want * 2 + 1)
    assert np.array_equal(x.cpu().numpy(), want)
