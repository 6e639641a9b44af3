"""Crops whose list lives on the device (``Decoder.bind`` ->
``CropBinding.decode_crops``) against the oracle's PCM through the definition
of test_gpu_decode_resample.py (``model_row``) and against
``Decoder.decode_crops`` on the same crops as a host list.  Every comparison is
exact: output bit-equal, written equal.  ``out`` is pre-filled with 0x5555
(float32: 0x55555555), so an element the kernel skipped shows.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle_ffi  # noqa: F401  (Res decodes through it)
from golden.cases import HERE
from test_crop_plan_shared import many_frames
from test_gpu_decode_resample import Res, craft, edge_crops, expected

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    import soundchunks_amd

    return soundchunks_amd


@pytest.fixture(scope="module")
def crafted(sc):
    """Mono and stereo streams of 4500 samples (ChunkSize 3, two frames around an empty one) per source rate."""
    made = {}

    def get(rate, ch):
        if (rate, ch) not in made:
            made[rate, ch] = Res(sc, craft(100 + rate % 97 + ch, ch, rate))
        return made[rate, ch]

    return get


def prefilled(shape, dtype, device):
    import torch

    if dtype == torch.float32:
        return torch.full(shape, 0x55555555, dtype=torch.int32, device=device).view(torch.float32)
    return torch.full(shape, 0x5555, dtype=torch.int16, device=device)


def check(sc, rs, crops, length, dtype=None, layout="TC", rate=None, channels=None, binding=None):
    """One bound call over pre-filled memory; the oracle's model and the host-planned call must both agree."""
    import torch

    dtype = torch.int16 if dtype is None else dtype
    b = sc.Decoder.bind([r.st for r in rs], rate=rate, channels=channels) if binding is None else binding
    want, lens, _ = expected(sc, rs, crops, length, dtype, layout, rate, channels)
    device = torch.device("cuda", rs[0].st.device)
    out = prefilled(want.shape, dtype, device)
    written = torch.full((len(crops),), -7, dtype=torch.int64, device=device)
    t = torch.tensor(crops, dtype=torch.int64, device=device).reshape(len(crops), 3)
    x, n = b.decode_crops(t, length, dtype=dtype, layout=layout, out=out, written=written)
    assert x is out and n is written
    got = x.cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (rate, channels, layout, len(bad), bad[:4].tolist(),
                           [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]])
    assert n.tolist() == lens, (n.tolist(), lens)
    xh, nh = sc.Decoder.decode_crops([r.st for r in rs], crops, length, dtype=dtype, layout=layout, rate=rate,
                                     channels=channels)
    assert torch.equal(x, xh) and n.tolist() == nh
    stats = b.last_call()
    assert stats["allocations"] == stats["copies"] == stats["synchronisations"] == 0 and stats["launches"] >= 1
    if binding is None:
        b.close()
    return x


@pytest.mark.parametrize("fmt", [("int16", "TC"), ("float32", "CT")])
@pytest.mark.parametrize("ch", [1, 2])
def test_native_rate(sc, crafted, ch, fmt):
    import torch

    r = crafted(32000, ch)
    crops, length = edge_crops(sc, len(r.ref), 32000, 32000)
    x = check(sc, [r], crops, length, getattr(torch, fmt[0]), fmt[1])
    assert not x[3].any()  # a crop behind the stream's end


@pytest.mark.parametrize("fmt", [("int16", "TC"), ("float32", "CT")])
@pytest.mark.parametrize("fi,fo,ch", [(32000, 44100, 1), (32000, 44100, 2), (48000, 44100, 2), (32000, 8000, 1)])
def test_format(sc, crafted, fi, fo, ch, fmt):
    import torch

    r = crafted(fi, ch)
    crops, length = edge_crops(sc, len(r.ref), fi, fo)
    assert length > 2 * sc.Decoder.resample_tile() and any(c == length for _, _, c in crops)
    check(sc, [r], crops, length, getattr(torch, fmt[0]), fmt[1], rate=fo)


def test_mixed_batch(sc):
    """Set members and a stream opened on its own, of different rates and channel counts, in one call."""
    import torch

    specs = [(26390, 1), (32000, 1), (44100, 2), (48000, 2)]
    gscs = [craft(200 + i, ch, rate, rows=(300, 350)) for i, (rate, ch) in enumerate(specs)]
    ss = sc.Decoder.open_many(gscs)
    rs = [Res(sc, g, st=ss[i]) for i, g in enumerate(gscs)]
    rs.append(Res(sc, craft(210, 1, 48000, rows=(300, 350))))
    n = len(rs[0].ref)
    crops = []
    for s in range(len(rs)):
        crops += [(s, 0, 1200), (s, n - 300, 1200), (s, 890, 40), (s, 3 * s + 1, 1), (s, n, 4)]
    rng = np.random.default_rng(5)
    crops = [crops[i] for i in rng.permutation(len(crops))]
    check(sc, rs, crops, 1200, torch.int16, "TC", rate=44100, channels=2)
    check(sc, rs, crops, 1200, torch.float32, "CT", rate=44100, channels=2)
    check(sc, rs, crops, 1200, torch.int16, "CT", rate=44100, channels=1)
    # the set's own method counts its members
    b = ss.bind(rate=44100, channels=2)
    check(sc, rs[:4], [(3, 5, 100), (0, 5, 100)], 100, rate=44100, channels=2, binding=b)
    b.close()
    rs[-1].st.close()
    ss.close()


@pytest.mark.parametrize("rate", [None, 44100])
def test_bad_crops(sc, crafted, rate):
    """All six kinds between good crops: their rows are zero, written -1, and the neighbours do not notice."""
    import torch

    rs = [crafted(32000, 2), crafted(48000, 2)]
    n, length = len(rs[0].ref), 700
    good = [(0, 10, 700), (1, 4000, 700), (0, 2090, 30), (1, n, 5), (0, n - 3, 9), (1, 100, 0), (0, 0, 1)]
    bad = [(-1, 0, 5), (2, 0, 5), (0, -1, 5), (1, n + 1, 0), (0, 5, -1), (1, 5, length + 1)]
    bad += [(1 << 40, 0, 5), (0, 1 << 62, 5), (0, 5, -(1 << 62))]
    crops, is_bad = [], []
    for i, g in enumerate(good):
        crops.append(g)
        is_bad.append(False)
        for c in bad[i::len(good)]:
            crops.append(c)
            is_bad.append(True)
    assert sum(is_bad) == len(bad)
    b = sc.Decoder.bind([r.st for r in rs], rate=rate)
    for dtype, layout in ((torch.int16, "TC"), (torch.float32, "CT")):
        device = torch.device("cuda", rs[0].st.device)
        shape = (len(crops), length, 2) if layout == "TC" else (len(crops), 2, length)
        out = prefilled(shape, dtype, device)
        t = torch.tensor(crops, dtype=torch.int64, device=device)
        x, w = b.decode_crops(t, length, dtype=dtype, layout=layout, out=out)
        xh, wh = sc.Decoder.decode_crops([r.st for r in rs], good, length, dtype=dtype, layout=layout, rate=rate)
        rows = torch.tensor(is_bad, device=device)
        assert not x[rows].any().item()
        assert (w[rows] == -1).all().item()
        assert torch.equal(x[~rows], xh) and w[~rows].tolist() == wh
    b.close()


@pytest.mark.parametrize("rate", [None, 44100])
def test_many_frames(sc, rate):
    """33 frames with runs of empty ones: a crop from every frame's first sample and one to every frame's last."""
    r = Res(sc, many_frames(rate=32000))
    first = [int(v) for v in r.st.index.first_sample]
    n, length = len(r.ref), 150
    assert r.st.frame_count == 33 and first[3] == 0 and first[30] == n
    crops = []
    for i in range(r.st.frame_count):
        crops.append((0, first[i], length if i % 2 else 40))
        if first[i + 1] > first[i]:
            c = min(first[i + 1], 50 + i)
            crops.append((0, first[i + 1] - c, c))
    check(sc, [r], crops, length, rate=rate)
    r.st.close()


@pytest.mark.parametrize("name", ["square_empty_frame0_cs4", "syn2s_cs7_mono_cbd12"])
def test_goldens(sc, name):
    r = Res(sc, (HERE / f"{name}.gsc").read_bytes())
    n = len(r.ref)
    rng = np.random.default_rng(len(name))
    length = 5000  # more than one tile of the fused kernel
    crops = [(0, int(b), int(c)) for b, c in zip(rng.integers(0, n + 1, 16), rng.integers(1, length + 1, 16))]
    check(sc, [r], crops, length)
    r.st.close()


def test_stream_order_and_reuse(sc, crafted):
    import torch

    r = crafted(32000, 2)
    n, length = len(r.ref), 600
    device = torch.device("cuda", r.st.device)
    lists = [[(0, 0, 600), (0, 3000, 600), (0, n - 100, 600)], [(0, 2000, 100), (0, 7, 600), (0, n, 3)]]
    want = [expected(sc, [r], c, length, torch.int16, "TC", None, None) for c in lists]
    b = sc.Decoder.bind([r.st])
    # one crop tensor rewritten in place between two calls, nothing synchronised in between
    src = [torch.tensor(c, dtype=torch.int64, device=device) for c in lists]
    t = torch.empty((3, 3), dtype=torch.int64, device=device)
    got = []
    for s in src:
        t.copy_(s)
        got.append(b.decode_crops(t, length))
    torch.cuda.synchronize()
    for (x, w), (xw, lens, _) in zip(got, want):
        assert np.array_equal(x.cpu().numpy(), xw) and w.tolist() == lens
    # the same binding from two streams, each with its own crops, out and written
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for s, c in zip(streams, src):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got.append(b.decode_crops(c, length, out=prefilled((3, length, 2), torch.int16, device)))
    for s in streams:
        s.synchronize()
    for (x, w), (xw, lens, _) in zip(got, want):
        assert np.array_equal(x.cpu().numpy(), xw) and w.tolist() == lens
    b.close()


def test_degenerate_shapes(sc, crafted):
    import torch

    r = crafted(32000, 2)
    device = torch.device("cuda", r.st.device)
    b = sc.Decoder.bind([r.st])
    x, w = b.decode_crops(torch.empty((0, 3), dtype=torch.int64, device=device), 64)
    assert tuple(x.shape) == (0, 64, 2) and tuple(w.shape) == (0,) and b.last_call()["launches"] == 0
    t = torch.tensor([(0, 5, 0), (0, 0, 0)], dtype=torch.int64, device=device)
    x, w = b.decode_crops(t, 0, layout="CT")
    assert tuple(x.shape) == (2, 2, 0) and w.tolist() == [0, 0] and b.last_call()["launches"] == 0
    x, w = b.decode_crops(t, 8)  # and the same crops with a length: one launch, rows of zeros
    assert b.last_call()["launches"] == 1 and not x.any().item() and w.tolist() == [0, 0]
    b.close()


def test_refusals(sc, crafted):
    import torch

    mono, stereo = crafted(32000, 1), crafted(32000, 2)
    device = torch.device("cuda", mono.st.device)
    with pytest.raises(sc.GscError, match=r"stream 1 has 2 channels"):
        sc.Decoder.bind([mono.st, stereo.st])
    with pytest.raises(sc.GscError, match=r"stream 1 has 2 channels.*3"):
        sc.Decoder.bind([mono.st, stereo.st], channels=3)
    with pytest.raises(sc.GscError, match=r"stream 0.*32000.*1000"):
        sc.Decoder.bind([mono.st], rate=1000)
    with pytest.raises(sc.GscError, match="no streams"):
        sc.Decoder.bind([])
    b = sc.Decoder.bind([stereo.st])
    t = torch.tensor([(0, 0, 10)], dtype=torch.int64, device=device)
    out = prefilled((1, 64, 2), torch.int16, device)
    calls = [dict(crops=[(0, 0, 10)]), dict(crops=t.cpu()), dict(crops=t.to(torch.int32)), dict(crops=t[:, :2]),
             dict(crops=t.reshape(3)), dict(crops=t, out=out.cpu()), dict(crops=t, out=out[:, :32]),
             dict(crops=t, dtype=torch.float16), dict(crops=t, layout="TCB"),
             dict(crops=t, written=torch.zeros(1, dtype=torch.int32, device=device))]
    for kw in calls:
        kw.setdefault("out", out)
        with pytest.raises(sc.GscError) as e:
            b.decode_crops(kw.pop("crops"), 64, **kw)
        assert str(e.value).strip(), kw
    with pytest.raises(sc.GscError, match="Decoder.decode_crops"):
        b.decode_crops([(0, 0, 10)], 64)
    torch.cuda.synchronize()
    assert (out == 0x5555).all().item()  # none of them wrote
    x, w = b.decode_crops(t, 64, out=out)  # and a correct call still works
    assert w.tolist() == [10] and np.array_equal(x[0, :10].cpu().numpy(), stereo.ref[:10])
    b.close()
    with pytest.raises(sc.GscError, match="closed"):
        b.decode_crops(t, 64)


def test_closed_streams(sc):
    """After a bound stream, or the set of one, is closed the call raises and launches nothing."""
    import torch

    gscs = [craft(300 + i, 2, 32000, rows=(100, 120)) for i in range(3)]
    ss = sc.Decoder.open_many(gscs[:2])
    single = sc.Decoder.open(gscs[2])
    device = torch.device("cuda", single.device)
    t = torch.tensor([(0, 0, 10), (2, 5, 10)], dtype=torch.int64, device=device)
    b1, b2 = sc.Decoder.bind(ss.streams + [single]), ss.bind()
    b1.decode_crops(t, 16)
    b2.decode_crops(t[:1], 16)
    single.close()
    with pytest.raises(sc.GscError, match="closed"):
        b1.decode_crops(t, 16)
    b2.decode_crops(t[:1], 16)  # the set is still open
    ss.close()
    with pytest.raises(sc.GscError, match="closed"):
        b2.decode_crops(t[:1], 16)
    b1.close()
    b2.close()
