"""Sample ranges of resident streams (``Decoder.open``, ``decode_samples``,
``Decoder.decode_crops``) against slices of the oracle's whole-stream decode
(``oracle_ffi.decode``), as int16 or as ``astype(float32) / 32768``.  Every
comparison is exact.  Crafted streams use StreamVersion 1, as in
test_gpu_decode.py; nothing is encoded here.
"""
from __future__ import annotations

import numpy as np
import pytest

import gsc_writer as gw
import oracle_ffi
from golden.cases import HERE

pytestmark = pytest.mark.gpu

GOLDENS = sorted(p.stem for p in HERE.glob("*.gsc"))


@pytest.fixture(scope="module")
def sc():
    import soundchunks_amd

    return soundchunks_amd


class Res:
    """A resident stream beside the oracle's PCM of the same bytes."""

    def __init__(self, sc, gsc):
        want, ch, rate = oracle_ffi.decode(gsc)
        self.ref = want.reshape(-1, ch)
        self.st = sc.Decoder.open(gsc)
        assert (self.st.channels, self.st.sample_rate, self.st.samples_per_channel) == (ch, rate, len(self.ref))


def _expected(rs, crops, length, dtype, layout):
    import torch

    ch = rs[0].ref.shape[1]
    want = np.zeros((len(crops), length, ch), np.int16)
    lens = []
    for i, (s, b, c) in enumerate(crops):
        part = rs[s].ref[b:b + c]
        want[i, :len(part)] = part
        lens.append(len(part))
    if dtype == torch.float32:
        want = want.astype(np.float32) / 32768
    return (want.transpose(0, 2, 1) if layout == "CT" else want), lens


def _check(sc, rs, crops, length, dtype=None, layout="TC", out=None):
    import torch

    dtype = torch.int16 if dtype is None else dtype
    x, n = sc.Decoder.decode_crops([r.st for r in rs], crops, length=length, dtype=dtype, layout=layout, out=out)
    want, lens = _expected(rs, crops, length, dtype, layout)
    assert x.is_cuda and x.dtype == dtype and tuple(x.shape) == want.shape and x.is_contiguous()
    assert n == lens
    got = x.cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (crops, length, layout, bad[:4].tolist())
    return x


def test_chunk_edges(sc):
    """ChunkSize 3, stereo: begin and end at offsets 0, 1, 2 inside a chunk,
    lengths 0, 1, 2, and chunks with the reverse flag set at both crop edges."""
    import torch

    rng = np.random.default_rng(41)
    count, cs = 50, 3
    syms = gw.random_symbols(rng, 2 * 40, count)
    for row in (4, 9):  # crops below start in chunk row 4 and end in chunk row 9: reversed on both channels
        for k in (0, 1):
            neg, _, hdr, idx = syms[2 * row + k]
            syms[2 * row + k] = (neg, 1, hdr, idx)
    r = Res(sc, gw.frame(syms, ch=2, count=count, cs=cs, att=rng.integers(0, 16, count),
                         codes=rng.integers(0, 256, (count, cs))))
    crops = [(0, 12 + bo, (27 + eo) - (12 + bo) + 1) for bo in range(3) for eo in range(3)]
    crops += [(0, b, n) for b in (12, 13, 14, 29) for n in (0, 1, 2)]
    _check(sc, [r], crops, 20)
    _check(sc, [r], crops, 20, torch.float32, "CT")


@pytest.mark.parametrize("policy", ["always", "once", "minimal"])
def test_checkpoint_edges(sc, policy):
    S = sc.Decoder.checkpoint_symbols()
    rng = np.random.default_rng(42)
    # mono, ChunkSize 3: symbol S starts at sample 3 * S
    mono = Res(sc, gw.random_frame(rng, 4 * S + 5, ch=1, count=600, cs=3, policy=policy))
    edge = 3 * S
    crops = [(0, edge + d, 7) for d in (-1, 0, 1)] + [(0, edge + d - 6, 7) for d in (-1, 0, 1)]
    crops.append((0, edge - 2, 2 * 3 * S + 4))  # segments 0 .. 2
    _check(sc, [mono], crops, 2 * 3 * S + 4)
    # 3 channels: S % 3 != 0, so a checkpoint falls inside a symbol row
    assert S % 3 != 0
    tri = Res(sc, gw.random_frame(rng, 3 * (S + 40), ch=3, count=70, cs=2, policy=policy))
    row = S // 3  # the row that holds symbols S - 1 and S
    crops = [(0, 2 * row + d, 5) for d in (-1, 0, 1, 2)] + [(0, 2 * row - 4 + d, 5) for d in (0, 1)]
    crops.append((0, 0, 2 * (S + 40)))
    _check(sc, [tri], crops, 2 * (S + 40), layout="CT")


def test_frame_edges(sc):
    """Frames that differ in ChunkSize, ChunkCount and bit depth (8, and 12 with
    an odd ChunkSize), with empty frames before, between and after."""
    import torch

    rng = np.random.default_rng(43)
    f0 = gw.random_frame(rng, 2 * 150, ch=2, count=64, cs=4, bd=8)           # 600 samples
    f1 = gw.random_frame(rng, 2 * 90, ch=2, count=300, cs=7, bd=12, adiv=9)  # 630 samples
    e = gw.random_frame(rng, 0, ch=2, count=5, cs=4)
    two = Res(sc, f0 + f1)
    crops = [(0, 590, 10), (0, 600, 10), (0, 595, 10), (0, 0, 1230), (0, 599, 1), (0, 599, 2)]
    _check(sc, [two], crops, 1230)
    _check(sc, [two], crops, 1230, torch.float32, "CT")
    gap = Res(sc, e + f0 + e + e + f1 + e)
    assert np.array_equal(gap.ref, two.ref)
    _check(sc, [gap], crops + [(0, 0, 5)], 1230)  # across the empty frames; from sample 0 with frame 0 empty


def test_clipping_and_refusals(sc):
    import torch

    rng = np.random.default_rng(44)
    r = Res(sc, gw.random_frame(rng, 2 * 100, ch=2, count=30, cs=5))   # 500 samples
    mono = Res(sc, gw.random_frame(rng, 100, ch=1, count=30, cs=5))
    n = 500
    good = [(0, n - 40, 40), (0, n - 10, 64), (0, n, 64), (0, n, 0), (0, 0, 0)]
    x = _check(sc, [r], good, 64)
    assert not x[2].any() and not x[1, 10:].any()
    out = torch.zeros((1, 64, 2), dtype=torch.int16, device=x.device)
    bad = [
        ([r], [(0, -1, 4)], 64, {}), ([r], [(0, n + 1, 0)], 64, {}), ([r], [(0, 0, -1)], 64, {}),
        ([r], [(0, 0, 65)], 64, {}), ([r], [(1, 0, 4)], 64, {}), ([r], [(-1, 0, 4)], 64, {}),
        ([r, mono], [(0, 0, 4)], 64, {}),
        ([r], [(0, 0, 4)], 64, dict(out=out.to(torch.float32))), ([r], [(0, 0, 4)], 64, dict(out=out[:, :32])),
        ([r], [(0, 0, 4)], 64, dict(out=out.cpu())), ([r], [(0, 0, 4)], 64, dict(out=out.transpose(1, 2))),
        ([r], [(0, 0, 4)], 64, dict(layout="TCB")), ([r], [(0, 0, 4)], 64, dict(dtype=torch.float16)),
    ]
    for streams, crops, length, kw in bad:
        with pytest.raises(sc.GscError) as e:
            sc.Decoder.decode_crops([s.st for s in streams], crops, length=length, **kw)
        assert str(e.value).strip(), (crops, kw)
        _check(sc, [r], good[:2], 64)  # and a correct call still works
    # the C entry point refuses a NULL destination
    import ctypes

    from soundchunks_amd import _lib

    hs = (ctypes.c_void_p * 1)(r.st._handle())
    cr = (_lib.GscCrop * 1)(_lib.GscCrop(0, 0, 4))
    assert sc.load().gsc_decode_crops(hs, 1, cr, 1, 0, 0, 64, None, None, None) < 0
    assert b"null" in sc.load().gsc_last_error()
    with pytest.raises(sc.GscError):
        r.st.decode_samples(n - 1, n + 1)
    assert r.st.decode_samples(n, n).shape == (0, 2)
    _check(sc, [r], good, 64)


@pytest.fixture(scope="module")
def pair(sc):
    rng = np.random.default_rng(45)
    a = Res(sc, gw.random_frame(rng, 2 * 700, ch=2, count=200, cs=4, rate=44100) +
            gw.random_frame(rng, 2 * 300, ch=2, count=77, cs=7, bd=12, rate=44100))
    b = Res(sc, gw.random_frame(rng, 2 * 400, ch=2, count=513, cs=9, bd=12, rate=48000))
    return a, b


BATCH = [(0, 100, 1000), (1, 0, 3600), (0, 100, 1000), (0, 600, 1000), (1, 3000, 777), (0, 2795, 33), (1, 5, 0),
         (0, 4000, 900)]


@pytest.mark.parametrize("layout", ["TC", "CT"])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_batch_of_two_streams(sc, pair, dtype, layout):
    """Different ChunkSize, bit depth and rate in one call; a repeated crop,
    overlapping crops, unequal counts under one length, one clipped crop."""
    import torch

    x = _check(sc, list(pair), BATCH, 3600, getattr(torch, dtype), layout)
    assert torch.equal(x[0], x[2])
    shape = (len(BATCH), 3600, 2) if layout == "TC" else (len(BATCH), 2, 3600)
    out = torch.full(shape, 7, dtype=getattr(torch, dtype), device=x.device)
    y = _check(sc, list(pair), BATCH, 3600, getattr(torch, dtype), layout, out=out)
    assert y is out and torch.equal(x, out)


def test_large_codebooks(sc, pair):
    """A 4096 x 16, 12-bit frame (132 KiB of tables), a small frame, then
    8191 x 16 (260 KiB, codebook offsets beyond 2^17) and another small one in
    one stream; then the two-stream batch as well."""
    import torch

    rng = np.random.default_rng(46)
    big = Res(sc, gw.random_frame(rng, 2 * 600, ch=2, count=4096, cs=16, bd=12, policy="once") +
              gw.random_frame(rng, 2 * 50, ch=2, count=40, cs=4) +
              gw.random_frame(rng, 2 * 40, ch=2, count=8191, cs=16, policy="once") +
              gw.random_frame(rng, 2 * 50, ch=2, count=9, cs=5, bd=12))
    # frames start at 0, 9600, 9800, 10440; 10690 samples
    crops = [(0, 0, 9600), (0, 9590, 20), (0, 4000, 3000), (0, 9700, 900), (0, 9799, 642), (0, 10400, 9000)]
    _check(sc, [big], crops, 9600)
    _check(sc, [big], crops, 9600, torch.float32, "CT")
    _check(sc, list(pair), BATCH, 3600, torch.float32, "CT")
    _check(sc, list(pair), BATCH, 3600)


def test_native_and_own_format_on_two_devices(sc):
    """The 4096 x 16, 12-bit frame (132 KiB of tables) resident on device 0,
    then on device 1, in one process: on each the native call, and the same
    crops with rate= the stream's own and channels= its own, which go through
    the resampling kernel, the one whose dynamic-LDS limit is raised per device."""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    rng = np.random.default_rng(46)
    gsc = gw.random_frame(rng, 2 * 600, ch=2, count=4096, cs=16, bd=12, policy="once")
    device = torch.cuda.current_device()
    crops = [(0, 0, 9600), (0, 9590, 10)]
    try:
        for d in (0, 1):
            torch.cuda.set_device(d)
            sc.set_device(d)
            r = Res(sc, gsc)
            assert r.st.device == d
            _check(sc, [r], crops, 9600)
            y, n = sc.Decoder.decode_crops([r.st], crops, length=9600, rate=r.st.sample_rate, channels=r.st.channels)
            want, lens = _expected([r], crops, 9600, torch.int16, "TC")
            assert y.dtype == torch.int16 and np.array_equal(y.cpu().numpy(), want) and n == lens
            r.st.close()
    finally:
        torch.cuda.set_device(device)
        sc.set_device(device)


def test_edges_of_mixed_frames(sc):
    """The chunk, checkpoint and frame edges again: frames of different
    ChunkSize, ChunkCount and bit depth (the 12-bit one with an odd ChunkSize in
    the middle, an `always`-checkpointed one) and empty frames inside one
    workgroup's run."""
    import torch

    S = sc.Decoder.checkpoint_symbols()
    rng = np.random.default_rng(48)
    f0 = gw.random_frame(rng, 2 * 150, ch=2, count=64, cs=4, bd=8)            # 600 samples
    f1 = gw.random_frame(rng, 2 * 90, ch=2, count=301, cs=7, bd=12, adiv=9)   # 630
    f2 = gw.random_frame(rng, 2 * 200, ch=2, count=513, cs=3, policy="always")  # 600
    e = gw.random_frame(rng, 0, ch=2, count=5, cs=4)
    r = Res(sc, e + f0 + e + f1 + f2 + e)
    crops = [(0, 590, 10), (0, 600, 10), (0, 595, 10), (0, 0, 1830), (0, 599, 1), (0, 1229, 2), (0, 1225, 700),
             (0, 1830, 5), (0, 3, 0)]
    _check(sc, [r], crops, 1830)
    _check(sc, [r], crops, 1830, torch.float32, "CT")
    # 3 channels and ChunkSize 1: a checkpoint inside a symbol row, and more symbols than samples per channel
    tri = Res(sc, gw.random_frame(rng, 3 * (70 * S + 5), ch=3, count=4000, cs=1, policy="minimal"))
    n = 70 * S + 5
    _check(sc, [tri], [(0, 0, n), (0, S // 3 - 1, 3), (0, 21 * S - 1, 2 * S), (0, n - 1, 1)], n, layout="CT")
    # mono, the three positions around symbol S, begin and end
    mono = Res(sc, gw.random_frame(rng, 4 * S + 5, ch=1, count=600, cs=3, policy="once"))
    edge = 3 * S
    _check(sc, [mono], [(0, edge + d, 7) for d in (-1, 0, 1)] + [(0, edge + d - 6, 7) for d in (-1, 0, 1)] +
           [(0, edge - 2, 6 * S + 4)], 6 * S + 4)


def test_residency(sc):
    """A crop call uploads its job descriptors and nothing of the stream."""
    rng = np.random.default_rng(47)
    short = gw.random_frame(rng, 2 * 1500, ch=2, count=100, cs=4)
    long_ = gw.random_frame(rng, 2 * 12000, ch=2, count=100, cs=4)
    assert len(long_) > 4 * len(short)
    a, b = Res(sc, short), Res(sc, long_)
    crops = [(0, 10, 2000), (0, 3000, 2500), (0, 5990, 100)]
    xa = _check(sc, [a], crops, 2500)
    ha = sc.Decoder.last_timing()["h2d_bytes"]
    xb = _check(sc, [b], crops, 2500)
    hb = sc.Decoder.last_timing()["h2d_bytes"]
    assert 0 < ha == hb < len(short)
    xa2 = _check(sc, [a], crops, 2500)
    assert (xa2 == xa).all().item() and not (xa == xb).all().item()


def test_stream_order(sc, pair):
    import torch

    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
    want, _ = _expected(pair, BATCH, 3600, torch.float32, "CT")
    with torch.cuda.stream(s):
        x, n = sc.Decoder.decode_crops([p.st for p in pair], BATCH, length=3600, dtype=torch.float32, layout="CT")
        y = x * 2 + 1
    s.synchronize()
    assert np.array_equal(y.cpu().numpy(), want * 2 + 1)
    assert np.array_equal(x.cpu().numpy(), want)


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_crops(sc, name):
    r = Res(sc, (HERE / f"{name}.gsc").read_bytes())
    n, ch = r.ref.shape
    rng = np.random.default_rng(len(name) + n)
    length = min(n, 3000)
    crops = [(0, int(b), int(c)) for b, c in zip(rng.integers(0, n, 5), rng.integers(1, length + 1, 5))]
    crops.append((0, max(n - length // 2, 0), length))
    for fs in r.st.index.first_sample[1:-1]:
        crops.append((0, max(int(fs) - length // 3, 0), length))
    _check(sc, [r], crops, length)
    _check(sc, [r], crops[:3], length, layout="CT")
    for _, b, c in crops[:3]:
        e = min(b + c, n)
        got = r.st.decode_samples(b, e)
        assert got.dtype == np.int16 and got.shape == (e - b, ch) and np.array_equal(got, r.ref[b:e])
    r.st.close()
