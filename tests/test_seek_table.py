"""Seek tables on the host (no GPU: ``Index.table()`` is host only): the layout
include/soundchunks.h documents, over every committed golden, the sanitizer
build of the table code, and that opening with a table never falls back to
the walk when there is no device."""
from __future__ import annotations

import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from golden.cases import HERE

ROOT = Path(__file__).resolve().parents[1]
GOLDENS = sorted(p.stem for p in HERE.glob("*.gsc"))


def parse_table(t: bytes):
    """(S, F, stream length, P, frame offsets, frame bit counts, checkpoints) at the documented offsets."""
    magic, version, S, F, length, P = struct.unpack_from("<4sIIIQQ", t, 0)
    assert magic == b"GSCT" and version == 1
    fr = np.frombuffer(t, dtype="<u8", count=2 * F, offset=32).reshape(F, 2)
    cps = np.frombuffer(t, dtype="<u8", count=P, offset=32 + 16 * F)
    return S, F, length, P, fr[:, 0], fr[:, 1], cps


@pytest.mark.parametrize("name", GOLDENS)
def test_table_layout(name):
    import soundchunks_amd as sc

    gsc = (HERE / f"{name}.gsc").read_bytes()
    ix = sc.Decoder.index(gsc)
    t = ix.table()
    assert t == ix.table() == sc.Decoder.index(gsc).table()
    S, F, length, P, off, nbits, cps = parse_table(t)
    assert len(t) == 32 + 16 * F + 8 * P
    assert S == sc.Decoder.checkpoint_symbols()
    assert F == ix.frame_count and length == len(gsc)
    assert np.array_equal(off.astype(np.int64), ix.byte_offset[:-1])
    per_frame = -(-(ix.frame_length * ix.channels) // S)
    assert P == int(per_frame.sum())
    # a frame's bitstream ends where the next frame starts (whole 16-bit words)
    assert np.all((nbits + 15) // 16 * 2 <= np.diff(ix.byte_offset).astype(np.uint64))
    first = np.concatenate(([0], np.cumsum(per_frame)))[:-1]
    for k in range(F):
        if per_frame[k]:
            assert cps[first[k]] == 0  # (bit 0, header -1)
            seg = cps[first[k]:first[k] + per_frame[k]]
            assert np.all(np.diff((seg >> np.uint64(3)).astype(np.int64)) >= 2 * S)  # a symbol has 2 bits or more
            assert np.all((seg & np.uint64(7)) <= 4) and np.all((seg >> np.uint64(3)) <= nbits[k])
        else:
            assert nbits[k] == 0


def test_table_check_under_sanitizers():
    """make table_check: index_table_write and the host half of index_from_table
    on exact-size heap copies of every golden and table, every cut and every
    header field, built with -fsanitize=address,undefined as a stand-alone program."""
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "soundchunks_amd" / "csrc"), "table_check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if "variants refused" in ln]
    assert len(lines) == len(GOLDENS), r.stdout[-2000:]


def test_table_needs_the_device_and_never_falls_back():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import soundchunks_amd as sc

    gsc = (HERE / "tiny_passthrough_cs8.gsc").read_bytes()
    t = sc.Decoder.index(gsc).table()
    with pytest.raises(sc.GscError, match="no HIP device|gfx950"):
        sc.Decoder.index(gsc, table=t)
    with pytest.raises(sc.GscError, match="no HIP device|gfx950"):
        sc.Decoder.open(gsc, table=t)
    # what the host can see of a bad table is refused before any device is asked for
    with pytest.raises(sc.GscError, match="seek table"):
        sc.Decoder.index(gsc, table=t[:-1])
    bad = bytearray(t)
    struct.pack_into("<I", bad, 8, 2 * sc.Decoder.checkpoint_symbols())
    with pytest.raises(sc.GscError, match="symbols per checkpoint"):
        sc.Decoder.index(gsc, table=bytes(bad))
