"""Stream fidelity (``CropBinding.fidelity``, ``Fidelity``) against the
definition of include/soundchunks.h applied in numpy int64 to the oracle's PCM
of the same bytes (``oracle_ffi.decode``) and the reference PCM.  Every
comparison is exact.  The outputs are pre-filled with 0x55 bytes, so a block the
kernel skipped shows.  Crafted streams are test_gpu_decode_resample.py's: 4500
samples, ChunkSize 3, frames of 2100, 0 and 2400 samples.
"""
from __future__ import annotations

import wave

import numpy as np
import pytest

import gsc_writer as gw
import oracle_ffi  # noqa: F401  (Res decodes with it)
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


def full_range(seed, n, ch):
    """A random int16 reference [n, ch] over the whole range without 0, so that every sample carries reference
    energy; it holds both ends of the range when it holds two samples."""
    ref = np.random.default_rng(seed).integers(-32768, 32768, (n, ch)).astype(np.int16)
    ref[ref == 0] = 1
    if n >= 2:
        ref[0, 0], ref[1, ch - 1] = -32768, 32767
    return ref


def model(x, ref, hop):
    """(err_energy, ref_energy, err_peak), int64 [nb] each, of int16 PCM x [S, C] against int16 ref [R, C] by the
    definition: the reference is zero from R on and ignored from S on."""
    S = len(x)
    r = np.zeros(x.shape, np.int64)
    n = min(S, len(ref))
    r[:n] = ref[:n]
    d = x.astype(np.int64) - r
    nb = -(-S // hop)
    pad = (0, nb * hop - S)
    e = np.pad((d * d).sum(axis=1), pad).reshape(nb, hop).sum(axis=1)
    q = np.pad((r * r).sum(axis=1), pad).reshape(nb, hop).sum(axis=1)
    p = np.pad(np.abs(d).max(axis=1, initial=0), pad).reshape(nb, hop).max(axis=1, initial=0)
    return e, q, p


def expected(rs, refs, hop):
    es, qs, ps = zip(*[model(r.ref, ref, hop) for r, ref in zip(rs, refs)])
    offsets = [0] + np.cumsum([len(e) for e in es]).tolist()
    return np.concatenate(es), np.concatenate(qs), np.concatenate(ps), offsets


def prefilled(n, dtype, device):
    import torch

    return torch.full((n * dtype.itemsize,), 0x55, dtype=torch.uint8, device=device).view(dtype)


def on_device(ref, device):
    import torch

    return torch.from_numpy(np.ascontiguousarray(ref)).to(device)


def check(sc, rs, refs, hop, binding=None, given=None):
    """One fidelity call over pre-filled memory against the model.  refs: numpy arrays, which go to the device
    first and are read in place (given: what the call gets instead).  Returns (Fidelity, the model's three)."""
    import torch

    b = sc.Decoder.bind([r.st for r in rs]) if binding is None else binding
    want_e, want_q, want_p, offsets = expected(rs, refs, hop)
    total = offsets[-1]
    outs = [prefilled(total, dt, b.device) for dt in (torch.int64, torch.int64, torch.int32)]
    if given is None:
        given = [on_device(ref, b.device) for ref in refs]
    fid = b.fidelity(given, hop, err_energy=outs[0], ref_energy=outs[1], err_peak=outs[2])
    if binding is None:
        b.close()
    assert fid.err_energy is outs[0] and fid.ref_energy is outs[1] and fid.err_peak is outs[2] and fid.hop == hop
    assert fid.offsets_host == offsets and fid.offsets.tolist() == offsets and len(fid) == total
    assert fid.samples == [len(r.ref) for r in rs] and fid.channels == [r.ch for r in rs]
    got_e, got_q, got_p = (t.cpu().numpy() for t in outs)
    bad = np.nonzero((got_e != want_e) | (got_q != want_q) | (got_p != want_p))[0]
    assert len(bad) == 0, (hop, len(bad), [(int(i), int(got_e[i]), int(want_e[i]), int(got_q[i]), int(want_q[i]),
                                            int(got_p[i]), int(want_p[i])) for i in bad[:4]])
    return fid, want_e, want_q, want_p


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("ch", [1, 2])
def test_crafted(sc, streams, ch, hop):
    r = streams(("craft", ch))
    assert len(r.ref) == 4500 and 2100 % hop != 0
    ref = full_range(10 * ch + 1, 4500, ch)
    assert ref.min() == -32768 and ref.max() == 32767
    fid, want_e, want_q, want_p = check(sc, [r], [ref], hop)
    assert len(fid) == -(-4500 // hop) and want_e.all() and want_q.all()
    e, q, p = fid.blocks(0)
    assert e.data_ptr() == fid.err_energy.data_ptr() and len(q) == len(p) == len(fid)


@pytest.mark.parametrize("hop", [64, 1000, 4097])
@pytest.mark.parametrize("ch", [1, 2])
def test_reference_is_the_pcm(sc, streams, ch, hop):
    """No error anywhere, so no wave has an error to add, and every wave still carries its reference energy,
    which is the envelope's energy."""
    r = streams(("craft", ch))
    fid, want_e, want_q, want_p = check(sc, [r], [r.ref], hop)
    assert not want_e.any() and not want_p.any() and want_q.all()
    assert not fid.err_energy.any() and not fid.err_peak.any()
    env = r.st.envelope(hop)
    assert fid.ref_energy.tolist() == env.energy.tolist()
    assert fid.snr_db().tolist() == [float("inf")] * len(fid) and fid.stream_snr_db().tolist() == [float("inf")]


def test_peak_65535(sc):
    """test_gpu_envelope.py's test_peak_32768 stream, which decodes -32768 at sample 521 (AttenuationDivider 2052,
    attenuation 1, 12-bit code 0), against 32767 everywhere: d = -65535 and d * d = 4,294,836,225 > 2^31."""
    rng = np.random.default_rng(7)
    count, cs = 3, 4
    codes = rng.integers(1800, 2300, (count, cs))
    codes[0, 1] = 0
    syms = gw.random_symbols(rng, 500, count)
    syms[130] = (0, 0, syms[130][2], 0)  # chunk 0, neither negated nor reversed: sample 130 * 4 + 1
    g = gw.frame(syms, ch=1, count=count, bd=12, cs=cs, rate=32000, adiv=2052, att=[1, 3, 5], codes=codes)
    r = Res(sc, g)
    assert len(r.ref) == 2000 and r.ref[521, 0] == -32768
    ref = np.full((2000, 1), 32767, np.int16)
    for hop in (64, 1024):
        fid, want_e, _, want_p = check(sc, [r], [ref], hop)
        blk = 521 // hop
        assert want_p[blk] == 65535 and int(fid.err_peak[blk]) == 65535
        assert want_e[blk] >= 4294836225 and int(fid.err_energy[blk]) == int(want_e[blk])
    r.st.close()


@pytest.mark.parametrize("R", [0, 1, 63, 64, 2100, 4499, 4500, 4600])
def test_reference_length(sc, streams, R):
    """The reference's end inside a wave, at a block edge, at a frame's end and past the stream; R = 0 is a null
    pointer."""
    for ch in (1, 2):
        r = streams(("craft", ch))
        ref = full_range(50 + R % 7 + ch, R, ch)
        for hop in (64, 1000):
            fid, _, want_q, _ = check(sc, [r], [ref], hop)
            # reference energy up to the block that holds sample R - 1 and nowhere after it
            last = -(-min(R, 4500) // hop)
            assert want_q[:last].all() and not want_q[last:].any()
            if R == 0:
                assert fid.err_energy.tolist() == r.st.envelope(hop).energy.tolist()


def test_two_byte_alignment(sc, streams):
    """The reference as a view that starts one int16 into its storage."""
    import torch

    for ch in (1, 2):
        r = streams(("craft", ch))
        ref = full_range(60 + ch, 4500, ch)
        b = sc.Decoder.bind([r.st])
        store = torch.zeros(4500 * ch + 1, dtype=torch.int16, device=b.device)
        view = store[1:].view(4500, ch)
        view.copy_(torch.from_numpy(ref))
        assert view.is_contiguous() and view.data_ptr() % 4 == 2 and view.data_ptr() == store.data_ptr() + 2
        check(sc, [r], [ref], 1000, binding=b, given=[view])
        b.close()


def test_numpy_references_are_uploaded(sc, streams):
    r = streams(("craft", 2))
    ref = full_range(70, 4400, 2)
    ref.setflags(write=False)
    check(sc, [r], [ref], 65, given=[ref])


def test_mixed_binding(sc):
    """Set members and a single open, of different rates and channel counts and with distinct references, in one
    binding whose rate and channel count change nothing: offsets and every block equal the per-stream calls."""
    specs = [(26390, 1), (32000, 2), (44100, 2)]
    gscs = [craft(320 + i, ch, rate, rows=(300 + 7 * i, 350)) for i, (rate, ch) in enumerate(specs)]
    ss = sc.Decoder.open_many(gscs)
    rs = [Res(sc, g, st=ss[i]) for i, g in enumerate(gscs)]
    rs.append(Res(sc, craft(330, 1, 48000, rows=(300, 351))))
    refs = [full_range(80 + i, len(r.ref) + (-5, 0, 9, -700)[i], r.ch) for i, r in enumerate(rs)]
    b = sc.Decoder.bind([r.st for r in rs], rate=16000, channels=1)
    for hop in (64, 1000):
        fid, _, _, _ = check(sc, rs, refs, hop, binding=b)
        for i, r in enumerate(rs):
            one = r.st.fidelity(refs[i], hop)
            for got, want in zip(fid.blocks(i), one.blocks(0)):
                assert got.tolist() == want.tolist()
        err, ref = fid.stream_sums()
        assert err.tolist() == [int(fid.blocks(i)[0].sum()) for i in range(4)]
        assert ref.tolist() == [int(fid.blocks(i)[1].sum()) for i in range(4)]
    b.close()
    ss.close()


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_golden(sc, streams, name, big):
    """Every sample of [0, S) meets its reference, the ones that decode to zero too: the reference has no zero."""
    r = streams(name)
    hop = GOLDENS[name] if big else 1024
    assert hop == 1024 or hop > 4096
    ref = full_range(90, len(r.ref), r.ch)
    _, want_e, want_q, _ = check(sc, [r], [ref], hop)
    assert want_e.all() and want_q.all()
    if hop == 1024 and name == "silence_tone_cs8_cpf256":
        silent = model(r.ref, np.zeros((0, r.ch), np.int16), hop)[0] == 0
        assert len(want_e) == 87 and int(silent.sum()) == 43
        assert (want_e[silent] == want_q[silent]).all()  # d = -r where the stream is silent
    if hop == 1024 and name == "tiny_passthrough_cs8":
        assert len(r.ref) == 888 and len(want_e) == 1


def test_hihat_against_its_wav(sc, streams):
    """Alignment and padding: stream sample t is WAV sample t, and the stream is padded past the WAV.  With the
    oracle's decoder on the CPU the pair gives 12.345 dB, -1.73 dB with the reference shifted by -1 sample and
    -1.71 dB with it shifted by +1; the order is asserted, not the decimals."""
    r = streams("hihat_cs8_cpf256")
    with wave.open(str(HERE / "lame_test_hihat.wav")) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (r.ch, 2, r.rate)
        pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, r.ch).astype(np.int16)
    assert (len(pcm), len(r.ref)) == (111605, 111608)
    fid, want_e, want_q, _ = check(sc, [r], [pcm], 1024)
    snr = float(fid.stream_snr_db()[0])
    assert snr == pytest.approx(10 * np.log10(int(want_q.sum()) / int(want_e.sum())), abs=1e-9)
    earlier = np.concatenate([pcm[1:], np.zeros((1, r.ch), np.int16)])  # reference sample t + 1 at t
    later = np.concatenate([np.zeros((1, r.ch), np.int16), pcm])  # reference sample t - 1 at t
    shifted = [float(check(sc, [r], [ref], 1024)[0].stream_snr_db()[0]) for ref in (earlier, later)]
    print(f"hihat_cs8_cpf256 against its WAV: {snr:.3f} dB; shifted by one sample: {shifted[0]:.3f} and "
          f"{shifted[1]:.3f} dB")
    assert snr > 0 and snr > shifted[0] and snr > shifted[1]
    s, first, worst = fid.worst(3)
    assert s.tolist() == [0] * 3 and all(f % 1024 == 0 and 0 <= f < 111608 for f in first.tolist())
    assert worst.tolist() == sorted(fid.snr_db().tolist())[:3]


def test_helpers_outlive_everything(sc):
    """ResidentStream.fidelity, Decoder.fidelity and StreamSet.fidelity bind for the call and close again; the
    Fidelity owns plain tensors."""
    g = craft(302, 2, 32000)
    st = sc.Decoder.open(g)
    r = Res(sc, g, st=st)
    ref = full_range(100, 4500, 2)
    want_e, want_q, want_p, offsets = expected([r], [ref], 1000)
    fids = [st.fidelity(ref, 1000), sc.Decoder.fidelity([st], [on_device(ref, "cuda")], 1000)]
    st.close()
    for fid in fids:
        assert fid.offsets_host == offsets
        assert fid.err_energy.cpu().numpy().tolist() == want_e.tolist()
        assert fid.ref_energy.cpu().numpy().tolist() == want_q.tolist()
        assert fid.err_peak.cpu().numpy().tolist() == want_p.tolist()
    gscs = [craft(310, 1, 32000, rows=(300, 350)), craft(311, 1, 44100, rows=(40, 30))]
    ss = sc.Decoder.open_many(gscs)
    rs = [Res(sc, g, st=ss[i]) for i, g in enumerate(gscs)]
    refs = [full_range(101 + i, len(r.ref), 1) for i, r in enumerate(rs)]
    want_e, want_q, want_p, offsets = expected(rs, refs, 64)
    fid = ss.fidelity(refs, 64)
    ss.close()
    assert fid.offsets_host == offsets and fid.err_energy.cpu().numpy().tolist() == want_e.tolist()
    assert fid.ref_energy.cpu().numpy().tolist() == want_q.tolist()
    assert fid.err_peak.cpu().numpy().tolist() == want_p.tolist()
    want = 10 * np.log10(np.add.reduceat(want_q, offsets[:-1]) / np.add.reduceat(want_e, offsets[:-1]))
    assert np.abs(fid.stream_snr_db().cpu().numpy() - want).max() <= 1e-9
    assert fid.worst(2)[2].tolist() == sorted(fid.snr_db().tolist())[:2]


def test_python_refusals(sc, streams):
    import torch

    r1, r2 = streams(("craft", 1)), streams(("craft", 2))
    b = sc.Decoder.bind([r2.st])
    dev = b.device
    good = on_device(full_range(110, 4500, 2), dev)
    with pytest.raises(sc.GscError, match="2 references for 1 streams"):
        b.fidelity([good, good])
    with pytest.raises(sc.GscError, match="0 references for 1 streams"):
        b.fidelity([])
    with pytest.raises(sc.GscError, match="reference 0 must be int16, got torch.int32"):
        b.fidelity([good.to(torch.int32)])
    with pytest.raises(sc.GscError, match="reference 0 must be int16, got float32"):
        b.fidelity([np.zeros((10, 2), np.float32)])
    with pytest.raises(sc.GscError, match=r"reference 0 must be \[R, 2\]"):
        b.fidelity([good[:, :1].contiguous()])
    with pytest.raises(sc.GscError, match=r"reference 0 must be \[R, 2\]"):
        b.fidelity([good.reshape(-1)])
    with pytest.raises(sc.GscError, match="reference 0 is not contiguous"):
        b.fidelity([on_device(np.zeros((100, 4), np.int16), dev)[:, ::2]])
    with pytest.raises(sc.GscError, match="reference 0 is not contiguous"):
        b.fidelity([np.zeros((100, 4), np.int16)[:, ::2]])
    with pytest.raises(sc.GscError, match="reference 0 is on cpu"):
        b.fidelity([good.cpu()])
    with pytest.raises(sc.GscError, match="reference 0 is list"):
        b.fidelity([[1, 2]])
    total = -(-4500 // 1024)
    with pytest.raises(sc.GscError, match="err_energy must be a contiguous torch.int64"):
        b.fidelity([good], err_energy=torch.zeros(total, dtype=torch.int32, device=dev))
    with pytest.raises(sc.GscError, match="ref_energy must be a contiguous torch.int64"):
        b.fidelity([good], ref_energy=torch.zeros(total + 1, dtype=torch.int64, device=dev))
    with pytest.raises(sc.GscError, match="err_peak must be a tensor on"):
        b.fidelity([good], err_peak=torch.zeros(total, dtype=torch.int32))
    for hop in (63, 65537):
        with pytest.raises(sc.GscError, match=f"hop {hop} outside"):
            b.fidelity([good], hop)
    # the second reference of two is the one named
    b2 = sc.Decoder.bind([r1.st, r2.st], channels=1)
    with pytest.raises(sc.GscError, match=r"reference 1 must be \[R, 2\], stream 1 has 2 channels"):
        b2.fidelity([np.zeros((5, 1), np.int16), np.zeros((5, 1), np.int16)])
    b2.close()
    # after the refusals the next good call is right
    check(sc, [r2], [good.cpu().numpy()], 1024, binding=b, given=[good])
    b.close()
    with pytest.raises(sc.GscError, match="the crop binding is closed"):
        b.fidelity([good])
    # a stream closed under its binding: raises, as decode_crops and envelope do
    own = sc.Decoder.open(craft(340, 1, 32000, rows=(40, 30)))
    b3 = sc.Decoder.bind([own])
    own.close()
    with pytest.raises(sc.GscError, match="a stream of the crop binding is closed"):
        b3.fidelity([np.zeros((5, 1), np.int16)])
    b3.close()
    with pytest.raises(sc.GscError, match="the resident stream is closed"):
        own.fidelity(np.zeros((5, 1), np.int16))


def test_library_refusals(sc, streams):
    """gsc_crop_binding_fidelity's own refusals, each naming what is at fault; nothing is launched by a refused
    call, and the next good call is right."""
    import ctypes

    import torch

    from soundchunks_amd import _lib

    r1, r2 = streams(("craft", 1)), streams(("craft", 2))
    rs = [r1, r2]
    b = sc.Decoder.bind([r.st for r in rs], channels=2)
    dev = b.device
    lib = _lib.load()
    total = 2 * -(-4500 // 1024)
    refs = [full_range(120 + i, 4500, r.ch) for i, r in enumerate(rs)]
    held = [on_device(ref, dev) for ref in refs]
    outs = [torch.full((total + 1,), 7, dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.int32)]
    host = np.zeros(4500 * 2, np.int16)

    def call(hop=1024, ptrs=None, lens=None, o=None, n=total, binding=b._h):
        ptrs = [t.data_ptr() for t in held] if ptrs is None else ptrs
        lens = [4500, 4500] if lens is None else lens
        o = [t.data_ptr() for t in outs] if o is None else o
        p = (ctypes.c_void_p * 2)(*ptrs) if ptrs != "null" else None
        ln = (ctypes.c_longlong * 2)(*lens) if lens != "null" else None
        rc = lib.gsc_crop_binding_fidelity(binding, hop, p, ln, o[0], o[1], o[2], n, None)
        return rc, lib.gsc_last_error()

    def refused(what, **kw):
        rc, msg = call(**kw)
        assert rc != 0 and what.encode() in msg, (what, rc, msg)

    # everything the envelope call refuses
    refused("binding is null", binding=None)
    refused("hop 63 outside", hop=63)
    refused("hop 65537 outside", hop=65537)
    for n in (total - 1, total + 1):
        refused(f"nblocks {n}, the binding's 2 streams have {total} blocks", n=n)
    good = [t.data_ptr() for t in outs]
    for i, name in enumerate(("err_energy_device", "ref_energy_device", "err_peak_device")):
        refused(f"{name} is null", o=good[:i] + [None] + good[i + 1:])
        refused(f"{name} is not device memory", o=good[:i] + [host.ctypes.data] + good[i + 1:])
    # the references
    refused("ref_device is null", ptrs="null")
    refused("ref_samples is null", lens="null")
    refused("stream 1: the reference has -1 samples", lens=[4500, -1])
    refused("stream 0: the reference has -4500 samples", lens=[-4500, -1])
    refused("stream 1: the reference is null and has 1 samples", ptrs=[held[0].data_ptr(), None], lens=[4500, 1])
    refused("stream 1: the reference is not device memory", ptrs=[held[0].data_ptr(), host.ctypes.data])
    refused("stream 0: the reference is not device memory", ptrs=[host.ctypes.data, host.ctypes.data])
    for t, dt in zip(outs, (torch.int64, torch.int64, torch.int32)):
        assert t.tolist() == [7] * (total + 1)  # nothing was launched
    # a good call through the same arrays, then through the binding's method
    rc, msg = call()
    assert rc == 0, msg
    want_e, want_q, want_p, _ = expected(rs, refs, 1024)
    assert outs[0][:total].tolist() == want_e.tolist() and outs[1][:total].tolist() == want_q.tolist()
    assert outs[2][:total].tolist() == want_p.tolist() and [int(t[total]) for t in outs] == [7] * 3
    # a null reference with 0 samples and a pointer with 0 samples are all-zero references
    rc, msg = call(ptrs=[None, held[1].data_ptr()], lens=[0, 0])
    assert rc == 0, msg
    zero = [np.zeros((0, r.ch), np.int16) for r in rs]
    want_e, want_q, want_p, _ = expected(rs, zero, 1024)
    assert outs[0][:total].tolist() == want_e.tolist() and not outs[1][:total].any()
    assert outs[2][:total].tolist() == want_p.tolist()
    check(sc, rs, refs, 1024, binding=b, given=held)
    b.close()
