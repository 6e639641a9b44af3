"""``Fidelity`` on CPU tensors with hand-made energies: the SNR formulas against
the same float64 formula in numpy (both sides evaluate one float64 expression
on integers below 2**56, so they agree within 1e-9 dB), the infinities, the
order of ``worst``, the views of ``blocks`` and the offsets of streams without
samples.  Host only: no device and no library call.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

HOP = 64
SAMPLES = [200, 0, 64, 0, 130]  # 4, 0, 1, 0 and 3 blocks
CHANNELS = [2, 1, 1, 2, 1]
OFFSETS = [0, 4, 4, 5, 5, 8]
#            stream 0                         stream 2   stream 4
ERR = [3, 0, (1 << 55) + 12345, 0,            977,       1, 5_000_000_007, 0]
REF = [1 << 40, 17, 999_999_999_989, 0,       0,         (1 << 55) + 1, 5_000_000_007, 0]
PEAK = [1, 0, 65535, 0,                       31,        1, 40000, 0]


@pytest.fixture(scope="module")
def fid():
    import soundchunks_amd as sc

    return sc.Fidelity(HOP, SAMPLES, CHANNELS, OFFSETS, torch.tensor(ERR, dtype=torch.int64),
                       torch.tensor(REF, dtype=torch.int64), torch.tensor(PEAK, dtype=torch.int32))


def snr_model(ref, err):
    """10 log10(ref / err) in float64; +inf where err is 0, -inf where only ref is."""
    ref, err = np.asarray(ref, np.int64), np.asarray(err, np.int64)
    out = np.full(len(err), np.inf)
    some = err != 0
    with np.errstate(divide="ignore"):
        out[some] = 10.0 * np.log10(ref[some].astype(np.float64) / err[some].astype(np.float64))
    return out


def assert_db(got, want):
    got = got.numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    inf = np.isinf(want)
    assert (np.isinf(got) == inf).all() and (got[inf] == want[inf]).all()  # the same infinities, the same signs
    assert not np.isnan(got).any()
    assert np.abs(got[~inf] - want[~inf]).max(initial=0.0) <= 1e-9


def test_members(fid):
    assert len(fid) == 8 and fid.hop == HOP
    assert fid.samples == SAMPLES and fid.channels == CHANNELS
    assert fid.offsets_host == OFFSETS and fid.offsets.tolist() == OFFSETS and fid.offsets.dtype == torch.int64
    assert fid.err_energy.tolist() == ERR and fid.ref_energy.tolist() == REF and fid.err_peak.tolist() == PEAK


def test_snr_db(fid):
    want = snr_model(REF, ERR)
    assert_db(fid.snr_db(), want)
    # err = 0 with and without reference energy: +inf; ref = 0 alone: -inf
    assert want[1] == np.inf and want[3] == np.inf and want[7] == np.inf and want[4] == -np.inf
    assert fid.snr_db()[[1, 3, 7]].tolist() == [float("inf")] * 3 and float(fid.snr_db()[4]) == float("-inf")
    assert np.isfinite(want[[0, 2, 5, 6]]).all() and want[6] == 0.0


def test_stream_snr_db(fid):
    err = [sum(ERR[a:b]) for a, b in zip(OFFSETS[:-1], OFFSETS[1:])]
    ref = [sum(REF[a:b]) for a, b in zip(OFFSETS[:-1], OFFSETS[1:])]
    assert max(err + ref) < 1 << 56
    e, r = fid.stream_sums()
    assert e.dtype == torch.int64 and e.tolist() == err and r.tolist() == ref  # exact
    want = snr_model(ref, err)
    assert_db(fid.stream_snr_db(), want)
    assert want[1] == np.inf and want[3] == np.inf and want[2] == -np.inf  # no samples: no error


def test_stream_sums_are_integer_exact():
    """Sums that float64 cannot hold: 2**55 + 1 three times is not a multiple of 4."""
    import soundchunks_amd as sc

    big = (1 << 55) + 1
    f = sc.Fidelity(HOP, [3 * HOP], [1], [0, 3], torch.tensor([big] * 3), torch.tensor([big, 0, 1]),
                    torch.zeros(3, dtype=torch.int32))
    e, r = f.stream_sums()
    assert e.tolist() == [3 * big] and r.tolist() == [big + 1]


def test_worst(fid):
    want = snr_model(REF, ERR)
    order = np.argsort(want, kind="stable")
    stream_of = np.repeat(np.arange(len(SAMPLES)), np.diff(OFFSETS))
    first_of = (np.arange(8) - np.asarray(OFFSETS)[stream_of]) * HOP
    for k in (0, 1, 3, 8, 20):
        s, first, snr = fid.worst(k)
        n = min(k, 8)
        assert len(s) == len(first) == len(snr) == n
        assert s.dtype == torch.int64 and first.dtype == torch.int64 and snr.dtype == torch.float64
        assert s.tolist() == stream_of[order[:n]].tolist()
        assert first.tolist() == first_of[order[:n]].tolist()
        assert_db(snr, want[order[:n]])
    # lowest first: the block with reference silence alone, then the finite ones rising, the infinities last in
    # block order
    s, first, snr = fid.worst(8)
    assert (s[0].item(), first[0].item()) == (2, 0)
    assert snr.tolist() == sorted(snr.tolist())
    assert list(zip(s.tolist(), first.tolist()))[-3:] == [(0, 64), (0, 192), (4, 128)]


def test_blocks(fid):
    for i, (a, b) in enumerate(zip(OFFSETS[:-1], OFFSETS[1:])):
        e, r, p = fid.blocks(i)
        assert e.tolist() == ERR[a:b] and r.tolist() == REF[a:b] and p.tolist() == PEAK[a:b]
        if b > a:  # views, not copies
            assert e.data_ptr() == fid.err_energy[a:].data_ptr() and p.data_ptr() == fid.err_peak[a:].data_ptr()
    assert len(fid.blocks(1)[0]) == 0 and len(fid.blocks(3)[2]) == 0
    assert fid.blocks(-1)[0].tolist() == ERR[5:]
    with pytest.raises(IndexError):
        fid.blocks(5)


def test_no_blocks_at_all():
    import soundchunks_amd as sc

    f = sc.Fidelity(HOP, [0, 0], [1, 2], [0, 0, 0], torch.zeros(0, dtype=torch.int64),
                    torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    assert len(f) == 0 and f.snr_db().shape == (0,)
    assert f.stream_snr_db().tolist() == [float("inf")] * 2
    assert [len(t) for t in f.worst(3)] == [0, 0, 0]
