"""Stream envelopes (``CropBinding.envelope``, ``Envelope``) against the
definition of include/soundchunks.h applied in numpy int64 to the oracle's PCM
of the same bytes (``oracle_ffi.decode``).  Every comparison is exact.  The
outputs are pre-filled with 0x55 bytes, so a block the kernel skipped shows.
Crafted streams are test_gpu_decode_resample.py's: 4500 samples, ChunkSize 3,
frames of 2100, 0 and 2400 samples.
"""
from __future__ import annotations

import numpy as np
import pytest

import gsc_writer as gw
import oracle_ffi
from golden.cases import HERE
from test_gpu_decode_resample import Res, craft

pytestmark = pytest.mark.gpu

HOPS = (64, 65, 1000, 4096, 4097, 65536)
GOLDENS = {"silence_tone_cs8_cpf256": 5000, "square_empty_frame0_cs4": 4097, "syn2s_cs7_mono_cbd12": 6000,
           "syn2s_c2_cs8_cpf4096": 65536, "tiny_passthrough_cs8": 4100}


@pytest.fixture(scope="module")
def sc():
    # torch before the library loads, as when the whole suite is collected (test_gpu_stream_set.py has the reason)
    import torch  # noqa: F401

    import soundchunks_amd

    return soundchunks_amd


@pytest.fixture(scope="module")
def streams(sc):
    """Resident streams beside the oracle's PCM, opened once: ("craft", ch) and goldens by name."""
    made = {}

    def get(key):
        if key not in made:
            gsc = craft(300 + key[1], key[1], 32000) if isinstance(key, tuple) else (HERE / f"{key}.gsc").read_bytes()
            made[key] = Res(sc, gsc)
        return made[key]

    return get


def model(ref, hop):
    """(energy int64 [nb], peak int64 [nb]) of int16 PCM [S, C] by the definition."""
    x = ref.astype(np.int64)
    n = len(x)
    nb = -(-n // hop)
    pad = (0, nb * hop - n)
    e = np.pad((x * x).sum(axis=1), pad).reshape(nb, hop).sum(axis=1)
    p = np.pad(np.abs(x).max(axis=1, initial=0), pad).reshape(nb, hop).max(axis=1, initial=0)
    return e, p


def expected(rs, hop):
    es, ps = zip(*[model(r.ref, hop) for r in rs])
    offsets = [0] + np.cumsum([len(e) for e in es]).tolist()
    return np.concatenate(es), np.concatenate(ps), offsets


def prefilled(n, dtype, device):
    import torch

    return torch.full((n * dtype.itemsize,), 0x55, dtype=torch.uint8, device=device).view(dtype)


def check(sc, rs, hop, binding=None):
    """One envelope call over pre-filled memory against the model; returns (Envelope, energy, peak) of the model."""
    import torch

    b = sc.Decoder.bind([r.st for r in rs]) if binding is None else binding
    want_e, want_p, offsets = expected(rs, hop)
    energy = prefilled(offsets[-1], torch.int64, b.device)
    peak = prefilled(offsets[-1], torch.int32, b.device)
    env = b.envelope(hop, energy=energy, peak=peak)
    if binding is None:
        b.close()
    assert env.energy is energy and env.peak is peak and env.hop == hop
    assert env.offsets_host == offsets and env.offsets.tolist() == offsets and len(env) == offsets[-1]
    assert env.samples == [len(r.ref) for r in rs] and env.channels == [r.ch for r in rs]
    got_e, got_p = energy.cpu().numpy(), peak.cpu().numpy()
    bad = np.nonzero((got_e != want_e) | (got_p != want_p))[0]
    assert len(bad) == 0, (hop, len(bad), [(int(i), int(got_e[i]), int(want_e[i]), int(got_p[i]), int(want_p[i]))
                                           for i in bad[:4]])
    return env, want_e, want_p


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("ch", [1, 2])
def test_crafted(sc, streams, ch, hop):
    r = streams(("craft", ch))
    assert len(r.ref) == 4500 and 2100 % hop != 0
    env, want_e, _ = check(sc, [r], hop)
    assert len(env) == -(-4500 // hop) and want_e.all()  # every block holds sound, the partial last one too
    if hop == 64:
        assert len(env) == 71
    e, p = env.blocks(0)
    assert e.data_ptr() == env.energy.data_ptr() and len(p) == len(env)


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_golden(sc, streams, name, big):
    r = streams(name)
    hop = GOLDENS[name] if big else 1024
    assert hop == 1024 or hop > 4096
    _, want_e, _ = check(sc, [r], hop)
    if hop == 1024:
        if name == "silence_tone_cs8_cpf256":
            assert len(want_e) == 87 and int((want_e == 0).sum()) == 43
        if name == "square_empty_frame0_cs4":
            assert 1055981997148 in want_e.tolist() and want_e.max() > 1 << 32
        if name == "tiny_passthrough_cs8":
            assert len(r.ref) == 888 and len(want_e) == 1


def test_stream_and_set_helpers(sc, streams):
    """ResidentStream.envelope, Decoder.envelope and StreamSet.envelope bind for the call and close again."""
    r = streams(("craft", 2))
    want_e, want_p, offsets = expected([r], 1000)
    for env in (r.st.envelope(1000), sc.Decoder.envelope([r.st], 1000)):
        assert env.offsets_host == offsets
        assert env.energy.cpu().numpy().tolist() == want_e.tolist()
        assert env.peak.cpu().numpy().tolist() == want_p.tolist()
    gscs = [craft(310, 1, 32000, rows=(300, 350)), craft(311, 1, 44100, rows=(40, 30))]
    ss = sc.Decoder.open_many(gscs)
    rs = [Res(sc, g, st=ss[i]) for i, g in enumerate(gscs)]
    want_e, want_p, offsets = expected(rs, 64)
    env = ss.envelope(64)
    ss.close()  # the envelope owns plain tensors
    assert env.offsets_host == offsets and env.energy.cpu().numpy().tolist() == want_e.tolist()
    assert env.peak.cpu().numpy().tolist() == want_p.tolist()


def test_peak_32768(sc):
    """A frame whose oracle PCM holds -32768: AttenuationDivider 2052, attenuation 1, 12-bit code 0 (-2048)
    gives CAttrLookup 524272 and (524272 * -2048) mod 2^32 >> 15 = 0x18000, low word 0x8000 (found by a
    search over the divider, the attenuation, the sign and the code on the CPU)."""
    rng = np.random.default_rng(7)
    count, cs = 3, 4
    codes = rng.integers(1800, 2300, (count, cs))
    codes[0, 1] = 0
    syms = gw.random_symbols(rng, 500, count)
    syms[130] = (0, 0, syms[130][2], 0)  # chunk 0, neither negated nor reversed: sample 130 * 4 + 1
    g = gw.frame(syms, ch=1, count=count, bd=12, cs=cs, rate=32000, adiv=2052, att=[1, 3, 5], codes=codes)
    r = Res(sc, g)
    assert len(r.ref) == 2000 and r.ref[521, 0] == -32768
    for hop in (64, 1024):
        env, _, want_p = check(sc, [r], hop)
        assert want_p[521 // hop] == 32768 and int(env.peak[521 // hop]) == 32768


def test_mixed_binding(sc):
    """Set members and a single open, of different rates and channel counts, in one binding whose rate and
    channel count change nothing: offsets and every block equal the per-stream calls."""
    specs = [(26390, 1), (32000, 2), (44100, 2)]
    gscs = [craft(320 + i, ch, rate, rows=(300 + 7 * i, 350)) for i, (rate, ch) in enumerate(specs)]
    ss = sc.Decoder.open_many(gscs)
    rs = [Res(sc, g, st=ss[i]) for i, g in enumerate(gscs)]
    rs.append(Res(sc, craft(330, 1, 48000, rows=(300, 351))))
    b = sc.Decoder.bind([r.st for r in rs], rate=16000, channels=1)
    for hop in (64, 1000):
        env, _, _ = check(sc, rs, hop, binding=b)
        for i, r in enumerate(rs):
            one = r.st.envelope(hop)
            e, p = env.blocks(i)
            assert e.tolist() == one.energy.tolist() and p.tolist() == one.peak.tolist()
    b.close()
    ss.close()


def test_refusals(sc, streams):
    import torch

    from soundchunks_amd import _lib

    r = streams(("craft", 1))
    b = sc.Decoder.bind([r.st])
    for hop in (63, 65537):
        with pytest.raises(sc.GscError, match=f"hop {hop} outside"):
            b.envelope(hop)
    total = -(-4500 // 1024)
    dev = b.device
    with pytest.raises(sc.GscError, match="energy must be a contiguous torch.int64"):
        b.envelope(1024, energy=torch.zeros(total, dtype=torch.int32, device=dev))
    with pytest.raises(sc.GscError, match="peak must be a contiguous torch.int32"):
        b.envelope(1024, peak=torch.zeros(total, dtype=torch.int64, device=dev))
    with pytest.raises(sc.GscError, match="peak must be a contiguous torch.int32"):
        b.envelope(1024, peak=torch.zeros(total + 1, dtype=torch.int32, device=dev))
    with pytest.raises(sc.GscError, match="energy must be a tensor on"):
        b.envelope(1024, energy=torch.zeros(total, dtype=torch.int64))
    # the library's own refusals: another nblocks, host memory, null
    lib = _lib.load()
    energy = torch.full((total + 1,), 7, dtype=torch.int64, device=dev)
    peak = torch.full((total + 1,), 7, dtype=torch.int32, device=dev)
    for n in (total - 1, total + 1):
        assert lib.gsc_crop_binding_envelope(b._h, 1024, energy.data_ptr(), peak.data_ptr(), n, None) != 0
        assert f"nblocks {n}, the binding's 1 streams have {total} blocks".encode() in lib.gsc_last_error()
    host = np.zeros(total, np.int64)
    assert lib.gsc_crop_binding_envelope(b._h, 1024, host.ctypes.data, peak.data_ptr(), total, None) != 0
    assert b"energy_device is not device memory" in lib.gsc_last_error()
    assert lib.gsc_crop_binding_envelope(b._h, 1024, energy.data_ptr(), None, total, None) != 0
    assert b"peak_device is null" in lib.gsc_last_error()
    assert lib.gsc_crop_binding_envelope(None, 1024, energy.data_ptr(), peak.data_ptr(), total, None) != 0
    assert energy.tolist() == [7] * (total + 1) and peak.tolist() == [7] * (total + 1)  # nothing was launched
    b.close()
    with pytest.raises(sc.GscError, match="the crop binding is closed"):
        b.envelope(1024)
    # a stream closed under its binding: raises, as decode_crops does
    own = sc.Decoder.open(craft(340, 1, 32000, rows=(40, 30)))
    b2 = sc.Decoder.bind([own])
    own.close()
    with pytest.raises(sc.GscError, match="a stream of the crop binding is closed"):
        b2.envelope(1024)
    b2.close()


def test_active(sc, streams):
    r = streams("silence_tone_cs8_cpf256")
    env, want_e, want_p = check(sc, [r], 1024)
    n, ch = len(r.ref), r.ch
    elems = np.minimum(1024, n - 1024 * np.arange(len(want_e))) * ch
    assert env.active().tolist() == (want_e > 0).tolist() and int(env.active().sum()) == 87 - 43
    for min_rms in (1, 100, 5000):
        want = want_e >= min_rms * min_rms * elems
        assert env.active(min_rms=min_rms).tolist() == want.tolist()
    assert 0 < int((want_e >= 100 * 100 * elems).sum()) < len(want_e)
    min_peak = int(np.median(want_p[want_p > 0]))
    want = want_p >= min_peak
    assert 0 < want.sum() < (want_p > 0).sum() + 1
    assert env.active(min_peak=min_peak).tolist() == want.tolist()
    both = (want_e >= 100 * 100 * elems) & want
    assert env.active(min_rms=100, min_peak=min_peak).tolist() == both.tolist()
    assert not env.active(min_peak=32769).any()


def test_sample_crops(sc, streams):
    import torch

    rs = [streams("silence_tone_cs8_cpf256"), streams("syn2s_c2_cs8_cpf4096")]
    assert (rs[0].ch, rs[1].ch, rs[0].rate) == (1, 2, rs[1].rate)
    b = sc.Decoder.bind([r.st for r in rs], channels=2)  # the mono stream's samples go to both channels
    env, want_e, _ = check(sc, rs, 1024, binding=b)
    gen = torch.Generator(device=b.device).manual_seed(11)
    span, n = 2000, 256
    crops = env.sample_crops(n, span, generator=gen)
    assert crops.device == b.device and crops.dtype == torch.int64 and tuple(crops.shape) == (n, 3)
    rows = crops.tolist()
    active = want_e > 0
    for s, begin, count in rows:
        assert s in (0, 1) and count == span
        ns = len(rs[s].ref)
        assert 0 <= begin <= max(ns - span, 0)
        b0, b1 = begin // 1024, -(-min(begin + span, ns) // 1024)
        assert active[env.offsets_host[s] + b0:env.offsets_host[s] + b1].any(), (s, begin)
    assert {s for s, _, _ in rows} == {0, 1}
    x, got = b.decode_crops(crops, span)
    assert got.tolist() == [span] * n
    assert bool(x.reshape(n, -1).any(dim=1).all())
    # the same seed draws the same crops
    again = env.sample_crops(n, span, generator=torch.Generator(device=b.device).manual_seed(11))
    assert torch.equal(again, crops)
    # count is copied to column 2
    assert env.sample_crops(4, span, count=900, generator=gen)[:, 2].tolist() == [900] * 4
    # nothing active: stream -1, which the bound call reports as -1 and a zero row
    none = env.sample_crops(8, span, min_peak=32769, generator=gen)
    assert none[:, 0].tolist() == [-1] * 8
    x, got = b.decode_crops(none, span)
    assert got.tolist() == [-1] * 8 and not x.any()
    # a span larger than the streams: begin 0
    wide = env.sample_crops(32, 10 ** 6, count=100, generator=gen)
    assert wide[:, 1].tolist() == [0] * 32 and set(wide[:, 0].tolist()) <= {0, 1}
    b.close()
