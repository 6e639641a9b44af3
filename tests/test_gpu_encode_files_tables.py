"""Per-file seek tables from the batch encoder:
``Prepared.encode_files(b, e, with_tables=True)`` returns the bytes and sizes
of ``encode_files(b, e)`` and, per file, the table the walk would write for
that file's bytes; the files and tables then open as one stream set."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARGV = ["-cs8", "-cpf256"]


@pytest.fixture(scope="module")
def sc():
    import torch  # noqa: F401  (before the library loads, as when the whole suite is collected)

    import soundchunks_amd

    return soundchunks_amd


@pytest.fixture(scope="module")
def batch(sc):
    from soundchunks_amd.synth import synth_wav

    # three short stereo inputs of different lengths (0.6 s is the smoke run's clip)
    p = sc.Encoder(ARGV).prepare_many([synth_wav(0.6), synth_wav(0.35), synth_wav(0.5)])
    yield p
    p.close()


def _cut(blob, sizes):
    out, o = [], 0
    for n in sizes:
        out.append(blob[o:o + n])
        o += n
    assert o == len(blob)
    return out


def test_tables_of_every_file(sc, batch):
    blob, sizes = batch.encode_files()
    blob_t, sizes_t, tables = batch.encode_files(with_tables=True)
    assert (blob_t, sizes_t) == (blob, sizes)
    assert len(tables) == len(sizes) == 3 and all(sizes)
    files = _cut(blob, sizes)
    for g, t in zip(files, tables):
        assert t == sc.Decoder.index(g).table()
    dec = sc.Decoder()
    ss = sc.Decoder.open_many(files, tables)
    try:
        for i, g in enumerate(files):
            want, rate = dec.decode(g)
            assert ss[i].sample_rate == rate
            assert np.array_equal(ss[i].decode_samples(0, ss[i].samples_per_channel), want), i
    finally:
        ss.close()


def test_a_range_that_leaves_out_the_last_file(sc, batch):
    first = [int(v) for v in batch.file_frames()]
    assert len(first) == 4 and first[2] < first[3]
    blob, sizes = batch.encode_files(0, first[2])
    blob_t, sizes_t, tables = batch.encode_files(0, first[2], with_tables=True)
    assert (blob_t, sizes_t) == (blob, sizes)
    assert sizes[2] == 0 and tables[2] == b"" and sizes[0] and sizes[1]
    for g, t in zip(_cut(blob, sizes)[:2], tables[:2]):
        assert t == sc.Decoder.index(g).table()
    # no frames at all: no bytes, and an empty table per file
    assert batch.encode_files(first[1], first[1], with_tables=True) == (b"", [0, 0, 0], [b"", b"", b""])
